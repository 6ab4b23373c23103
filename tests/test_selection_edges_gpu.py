"""Every top-k selection path held to an exact model on distances the test controls bit for bit (selection_ref.py): a one-hot query
under the dot metric makes column j of the store the distance array, so ties, byte carries, negative and non-finite distances sit at
the ranks the test chooses. ids, scores and counts of every answer equal the model's, with no tolerance, on
  (a) the default route, (b) "select_short" 0, (c) "force_general" 1 (the radix passes also for k <= 192), (d) (c) under "select_grid"
  4 and 1 (the multi-trip loops of select_hist_kernel / select_compact_kernel and their `n % 4` tail on 70 001 rows),
at row_base 0, 0x00FFFF00 and 0xFFFE0000, for the batched path, and once at the production grid on 6 291 463 rows.
test_selection_edges_cpu.py proves that each construction has the property its case needs and names the case that notices each
reverted line of the radix kernels."""
import time

import numpy as np
import pytest

import selection_ref as R

pytestmark = pytest.mark.gpu

ROUTES = (("default", 1, 0, 0), ("select_short-0", 0, 0, 0), ("force_general", 1, 1, 0), ("force_general-grid4", 1, 1, 4),
          ("force_general-grid1", 1, 1, 1))


@pytest.fixture(scope="module")
def wax(hip_lib):
    import wax_amd
    if hip_lib.wax_hip_device_count() == 0:
        pytest.skip("no HIP device on this host: the gpu-marked tests run on the MI355X box (pytest -m gpu)")
    assert hip_lib.wax_hip_available() == 1, "a HIP device is visible but it is not gfx950: the HIP path needs an MI355X"
    return wax_amd


@pytest.fixture(scope="module")
def loaded(wax):
    """name -> (engine, columns): every store is built and uploaded once per module."""
    cache = {}

    def get(name):
        if name not in cache:
            metric, rows, cols = R.build_store(name)
            eng = wax.HIPVectorEngine(metric=wax.VectorMetric(metric), dimensions=rows.shape[1])
            eng.addBatch(R.frame_ids(len(rows)), rows)
            cache[name] = (eng, cols)
        eng = cache[name][0]
        set_route(eng, ROUTES[0])                                    # whatever an earlier (failed) test left set
        eng.setRowBase(0)
        return cache[name]
    return get


def set_route(eng, route):
    _, short, general, grid = route
    eng.setTuning("select_short", short)
    eng.setTuning("force_general", general)
    eng.setTuning("select_grid", grid)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_answer(got, want, ctx):
    assert len(got[0]) == len(want[0]), f"{ctx}: {len(got[0])} results, the model has {len(want[0])}"
    if not np.array_equal(got[0], want[0]):
        at = int(np.nonzero(got[0] != want[0])[0][0])
        raise AssertionError(f"{ctx}: ids differ from rank {at + 1}: {got[0][at:at + 4]} vs {want[0][at:at + 4]}")
    assert np.array_equal(bits(got[1]), bits(want[1])), f"{ctx}: scores differ"


def route_counters(eng):
    return eng.getTuning("short_selects"), eng.getTuning("short_select_failures"), eng.getTuning("merged_scans")


def check_route_counters(eng, route, k, before, ctx):
    """The route taken, from "short_selects" / "short_select_failures" / "merged_scans", against the rules of search_internal.inc
    restated in selection_ref.py (expected_route). A short selection that fails (ties that bunch in one workgroup's lists) is
    legitimate here: the answer behind it is held to the model like any other."""
    name, short, general, _ = route
    k_eff = min(R.clamp_topk(k), eng.count)
    after = route_counters(eng)
    tried, failed, merged = (a - b for a, b in zip(after, before))
    want_tried, want_merged = R.expected_route(k_eff, eng.count, eng.dimensions, eng.getTuning("scan_grid"), short, general)
    assert (tried, merged) == (want_tried, want_merged), (ctx, tried, merged, want_tried, want_merged, eng.getTuning("scan_grid"))
    assert 0 <= failed <= tried, (ctx, tried, failed)                # (a short merge fails too when the tied prefixes overflow its LDS buffer: `flat`)
    return tried, failed


CASES = [(s, c) for s in R.STORE_NAMES for c in R.STORE_COLUMNS[s]]


@pytest.mark.parametrize("store,column", CASES, ids=[f"{s}-{c}" for s, c in CASES])
def test_every_route_equals_the_model(loaded, store, column):
    eng, cols = loaded(store)
    q, col, extra = cols[column]
    tally = {}
    try:
        for rb in R.row_bases_for(col.n):
            eng.setRowBase(rb)
            for k in R.ks_of(column, col, extra):
                want = col.answer(k, rb)
                for route in ROUTES:
                    set_route(eng, route)
                    ctx = f"{store} {column} k={k} row_base={rb:#x} {route[0]}"
                    before = route_counters(eng)
                    got = eng.searchArrays(q, k)
                    assert_answer(got, want, ctx)
                    tried, failed = check_route_counters(eng, route, k, before, ctx)
                    t = tally.setdefault(route[0], [0, 0, 0])
                    t[0] += 1
                    t[1] += tried
                    t[2] += failed
    finally:
        set_route(eng, ROUTES[0])
        eng.setRowBase(0)
    print(f"{store} {column}: " + ", ".join(f"{r}: {t[0]} answers, {t[1]} short selections, {t[2]} failed" for r, t in tally.items()))


def test_the_short_selection_answers_where_it_should(loaded):
    """Route (a) must not be the long path under another name. 70 001 >= 256 * 193: at k = 193 the default route tries the short
    selection, at 64- and at 5-d, and on the shuffled columns (`wide`, `ladder-low-byte`: their best rows are spread over the
    workgroups' lists) its certificate holds, so the short selection's own hits are what the model is compared with. At 64-d the scan
    grid is above 160 workgroups, so k = 65 and 192 go through the same kernel as the short merge; the 5-d stores merge in the scan
    kernel (that the counters follow these rules in every case of the matrix is asserted there)."""
    for store in ("dot-70001x64", "dot-70001x5-a"):
        eng, cols = loaded(store)
        grid = eng.getTuning("scan_grid")
        assert R.tries_short(193, eng.count, grid), (store, grid)
        assert not R.tries_short(1000, eng.count, grid)
    eng, cols = loaded("dot-70001x64")
    grid = eng.getTuning("scan_grid")
    assert grid > R.SCAN_FUSE_MERGE_GRID, grid
    for column in ("wide", "ladder-low-byte"):
        q, col, _ = cols[column]
        for k in (65, 192, 193):
            assert R.expected_route(k, eng.count, 64, grid, 1, 0) == (1, 0)
            before = route_counters(eng)
            got = eng.searchArrays(q, k)
            tried, failed, merged = (a - b for a, b in zip(route_counters(eng), before))
            assert (tried, failed, merged) == (1, 0, 0), (column, k, tried, failed, merged)
            assert_answer(got, col.answer(k), f"dot-70001x64 {column} k={k}: the short selection's own answer")


@pytest.mark.parametrize("store", R.STORE_NAMES)
def test_batched_path_equals_the_model(loaded, store):
    """searchBatch of 32 queries, every distribution of the store several times and interleaved, k = 10 and 100: the model's answer
    per query. (Ties send queries to the exact fallback; only the answers are asserted.)"""
    eng, cols = loaded(store)
    names = list(cols)
    order = [names[i % len(names)] for i in range(32)]
    queries = np.stack([cols[c][0] for c in order])
    n = eng.count
    try:
        for rb in R.row_bases_for(n)[:2]:
            eng.setRowBase(rb)
            for k in (10, 100):
                ids, scores, counts = eng.searchBatch(queries, k)
                for i, c in enumerate(order):
                    want = cols[c][1].answer(k, rb)
                    m = int(counts[i])
                    assert_answer((ids[i, :m], scores[i, :m]), want, f"{store} batch query {i} ({c}) k={k} row_base={rb:#x}")
    finally:
        eng.setRowBase(0)


def test_default_grid_on_6291463_rows(wax):
    """The one large case: 6 291 463 x 4 (dot), the smallest row count at which the four-deep loop of select_hist_kernel runs under the
    production grid of 2 048 workgroups, and no multiple of 4. Column 0: iid uniform x in [0, 1) (d = 1 - x; 2^24 values over 6.3M
    rows, so equal distances are everywhere) with 300 000 rows forced to d = 0.75; column 1: every d = 0.75, so the answer is rows
    0 .. k - 1, decided in the row digits over the whole store (the case that notices the four-deep loop's row index at this grid:
    test_selection_edges_cpu.py). k = 300 and 10 000 with "select_short" 0 and 1, against the model. On column 0 (shuffled) the short
    selection at k = 300 must certify its answer. Measured on one MI355X: 0.8 s wall, 0.7 s of it building the store and its model
    (test_k_sweep_fused_and_general_paths, 17 cases: 0.3 s of calls behind a 1.7 s module setup)."""
    import torch
    t0 = time.perf_counter()
    dev = torch.device("cuda", 0)
    n = R.BIG_N
    g = torch.Generator(device=dev)
    g.manual_seed(20265)
    rows = torch.randn((n, 4), generator=g, device=dev, dtype=torch.float32)
    rows[:, 0] = torch.rand((n,), generator=g, device=dev, dtype=torch.float32)
    forced = torch.randperm(n, generator=g, device=dev)[:R.BIG_FORCED]
    rows[forced, 0] = 0.25
    rows[:, 1] = 0.25
    ids = np.arange(n, dtype=np.uint64) + np.uint64(5)
    eng = wax.HIPVectorEngine(metric=wax.VectorMetric(1), dimensions=4)
    eng.addBatchDevice(ids, rows.contiguous())
    x0 = rows[:, 0].cpu().numpy()
    del rows
    d0 = R.dot_distance(x0)
    assert int(np.sum(d0 == np.float32(0.75))) >= R.BIG_FORCED and 0.0 < d0.min() and d0.max() <= 1.0
    columns = {0: d0, 1: np.full(n, 0.75, dtype=np.float32)}
    t1 = time.perf_counter()
    for j, d in columns.items():
        u = R.ukeys(d, 0)
        top = np.argpartition(u, 10000)[:10001]
        top = top[np.argsort(u[top])]
        for k in (300, 10000):
            want = (ids[top[:k]], -d[top[:k]])
            for short in (0, 1):
                eng.setTuning("select_short", short)
                before = route_counters(eng)
                got = eng.searchArrays(R.one_hot(4, j), k)
                ctx = f"6291463 x 4 column {j} k={k} select_short={short}"
                assert_answer(got, want, ctx)
                tried, failed, merged = (a - b for a, b in zip(route_counters(eng), before))
                assert (tried, merged) == R.expected_route(k, n, 4, eng.getTuning("scan_grid"), short, 0), (ctx, tried, merged)
                assert 0 <= failed <= tried, (ctx, tried, failed)
                if j == 0 and short and k == 300:
                    assert (tried, failed) == (1, 0), (ctx, tried, failed)      # the certificate path answered
                print(f"{ctx}: {tried} short selections, {failed} failed")
    print(f"default-grid case: {time.perf_counter() - t0:.2f} s wall ({t1 - t0:.2f} s to build the store and its model)")


def test_select_grid_key(wax):
    eng = wax.HIPVectorEngine(metric=wax.VectorMetric(1), dimensions=4)
    assert eng.getTuning("select_grid") == 0
    for bad in (-1, 2049):
        with pytest.raises(wax.EncodingError, match="select_grid must be"):
            eng.setTuning("select_grid", bad)
    for v in (2048, 1, 0):
        eng.setTuning("select_grid", v)
        assert eng.getTuning("select_grid") == v
