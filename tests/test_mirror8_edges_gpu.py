"""The 8-bit code mirror itself, held to float64 ("Eight bits per element"). An answer from it is released only when
`lb_KP - slack > d_k`, which needs every row's key to be a lower bound of its exact distance — so the codes, the scale, the err,
the key arithmetic and the upkeep of all of it are checked here directly, through `mirror8Snapshot` (what the device holds) and through
stores on which a lost, halved or partly summed err changes the answer or the certificate:
  (a) the conversion kernel, row by row, on every store the other mirror8 file uses and on rows f32 squares cannot hold;
  (b) the mirror after every kind of mutation;
  (c) a row whose quantisation error is aligned with the query;
  (d) the certificate decision on a ladder of rows a few slacks apart;
  (e) the row-count edges of the scan.
The constructions, the f64 arithmetic (`check_rows`) and the CPU model are in mirror8_ref.py; test_mirror8_cpu.py proves what each
construction must have for its GPU test to be able to fail. Every engine here runs "mirror_bits" 8 under "scan_mirror" 2."""
import numpy as np
import pytest

import oracle
import mirror8_ref as R
from helpers import OracleEngine, assert_parity

pytestmark = pytest.mark.gpu

C8 = ("mirror8_passes", "mirror8_fallbacks", "mirror8_unavailable", "mirror8_conversions", "mirror8_rows_converted",
      "mirror8_breaker_trips", "mirror_scans", "mirror_passes")


@pytest.fixture(scope="module")
def wax(hip_lib):
    import wax_amd
    if hip_lib.wax_hip_device_count() == 0:
        pytest.skip("no HIP device on this host: the gpu-marked tests run on the MI355X box (pytest -m gpu)")
    assert hip_lib.wax_hip_available() == 1, "a HIP device is visible but it is not gfx950: the HIP path needs an MI355X"
    return wax_amd


def make_engine(wax, metric, dims, corpus, ids=None):
    eng = wax.HIPVectorEngine(metric=wax.VectorMetric(metric), dimensions=dims)
    eng.addBatch(np.arange(len(corpus), dtype=np.uint64) if ids is None else ids, corpus)
    eng.setTuning("mirror_bits", 8)
    return eng


def counters(eng):
    return {n: eng.getTuning(n) for n in C8}


def delta(eng, before):
    after = counters(eng)
    return {n: after[n] - before[n] for n in C8}


def answer(eng, q, k, mode):
    eng.setTuning("scan_mirror", mode)
    return eng.searchArrays(q, k)


def same(a, b):
    return np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1], equal_nan=True)


def warm(eng, q, k=10):
    """Three eligible queries: two on bf16, the third builds the code mirror and rides it."""
    c = counters(eng)
    for _ in range(3):
        answer(eng, q, k, 2)
    d = delta(eng, c)
    assert (d["mirror8_passes"], d["mirror8_conversions"], d["mirror_scans"]) == (1, 1, 3), d
    return d


def one_case(eng, q, k, ctx):
    """One blocking query on the code mirror: (answer, certified). The answer is the f32 scan's, the pass was the code mirror's."""
    c = counters(eng)
    got = answer(eng, q, k, 2)
    d = delta(eng, c)
    assert (d["mirror8_passes"], d["mirror_passes"], d["mirror8_unavailable"], d["mirror8_conversions"]) == (1, 1, 0, 0), (ctx, d)
    assert d["mirror8_fallbacks"] in (0, 1), (ctx, d)
    assert same(got, answer(eng, q, k, 0)), f"{ctx}: not the f32 scan's answer"
    return got, d["mirror8_fallbacks"] == 0


def check_mirror(eng, rows, metric, ctx):
    """Everything (a) asks of the whole mirror against the f64 rows it must have been made from."""
    codes, scale, err, max_norm, coded = eng.mirror8Snapshot()
    assert coded == eng.count == len(rows) == len(codes), (ctx, coded, eng.count, len(rows))
    classes = R.check_rows(rows, metric, codes, scale, err, ctx)
    R.check_max_norm(rows, max_norm, ctx)
    head = eng.mirror8Snapshot(0, 0)                                 # no rows: the two words only
    assert head[0].shape == (0, rows.shape[1]) and head[3] == max_norm and head[4] == coded
    return classes


def refused(wax, eng, ctx):
    with pytest.raises(wax.EncodingError, match="code mirror is absent or not valid"):
        eng.mirror8Snapshot(0, 0)
    with pytest.raises(wax.EncodingError, match="code mirror is absent or not valid"):
        eng.mirror8Snapshot()


# ---- (a) the conversion kernel against f64, row by row --------------------------------------------------------------------------

STORES = {
    "gaussian-cosine-20005x384": lambda: (R.corpus_for(0, 20005, 384), 0),
    "gaussian-dot-20005x384": lambda: (R.corpus_for(1, 20005, 384), 1),
    "gaussian-cosine-5003x768": lambda: (R.corpus_for(0, 5003, 768), 0),
    "gaussian-dot-5003x768": lambda: (R.corpus_for(1, 5003, 768), 1),
    "outlier-element": lambda: (R.outlier_store(), 0),
    "zero-rows": lambda: (R.zero_row_store(), 0),
    "inf-nan-zero-cosine": lambda: (R.non_finite_store(0), 0),
    "inf-nan-zero-dot": lambda: (R.non_finite_store(1), 1),
    "subnormal-huge-flat-dot": lambda: (R.extreme_dot_store(), 1),
}
EXPECTED_CLASSES = {"zero-rows": (5020, 4980, 0), "inf-nan-zero-cosine": (4901, 101, 1), "inf-nan-zero-dot": (5001, 0, 2)}


@pytest.mark.parametrize("name", list(STORES))
def test_conversion_kernel_against_f64_row_by_row(wax, name):
    """Codes, scale, soundness and tightness of err, the rows that cannot be coded, the cosine zero rows and the max-norm word of the
    whole mirror, as R.check_rows / R.check_max_norm state them."""
    rows, metric = STORES[name]()
    eng = make_engine(wax, metric, rows.shape[1], rows)
    d = warm(eng, R.queries_for(rows.shape[1])[0])
    assert d["mirror8_rows_converted"] == len(rows)
    classes = check_mirror(eng, rows, metric, name)
    want = EXPECTED_CLASSES.get(name, (len(rows), 0, 0))
    assert (classes["coded"], classes["zero"], classes["lost"]) == want, classes
    if name == "subnormal-huge-flat-dot":
        codes = eng.mirror8Snapshot(R.EXTREME_FLAT, 1)[0]
        assert set(np.unique(codes)) == {1, 255}                    # every element is +-max
    with pytest.raises(wax.EncodingError, match="exceed"):
        eng.mirror8Snapshot(len(rows), 1)
    with pytest.raises(wax.EncodingError, match="exceed"):
        eng.mirror8Snapshot(1, len(rows))


@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 256, 257, 16385, 65553])
def test_conversion_kernel_row_counts(wax, n):
    """A workgroup per 16-row tile, its four waves rows 4 j + w of the tile in four steps, at most 4 096 workgroups: the small counts
    leave waves, steps and most of the only tile without a row, 255 to 257 rows end before, at and behind a tile's last row, 16 385
    rows are 1 025 workgroups of one tile each (the last tile a single row), and 65 553 rows are 4 098 tiles, so workgroups 0 and 1
    take a second tile, the last one ragged. Every row is written (each satisfies (a)); as an append onto 64 coded rows the same
    count must leave those 64 byte for byte as they were. (What lies beyond the last coded row cannot be read: the snapshot refuses
    the range.)"""
    dims = 384
    queries = R.queries_for(dims)
    rows = R.corpus_for(0, n, dims, seed=83)
    eng = make_engine(wax, 0, dims, rows)
    warm(eng, queries[0])
    check_mirror(eng, rows, 0, f"{n} rows")
    if n > 257:
        return
    base = R.corpus_for(0, 64, dims, seed=85)
    eng = wax.HIPVectorEngine(metric=wax.VectorMetric(0), dimensions=dims)
    eng.reserve(64 + n)                                              # no new slab at the append: only the appended rows are converted
    eng.addBatch(np.arange(64, dtype=np.uint64), base)
    eng.setTuning("mirror_bits", 8)
    warm(eng, queries[0])
    before = eng.mirror8Snapshot()
    eng.addBatch(np.arange(1000, 1000 + n, dtype=np.uint64), rows)
    c = counters(eng)
    answer(eng, queries[0], 10, 2)
    d = delta(eng, c)
    assert (d["mirror8_conversions"], d["mirror8_rows_converted"], d["mirror8_passes"]) == (1, n, 1), d
    after = eng.mirror8Snapshot()
    assert after[4] == 64 + n
    for a, b in zip(before[:3], after[:3]):
        assert np.array_equal(a.view(np.uint8), b[:64].view(np.uint8)), f"append of {n}: the rows coded before it changed"
    check_mirror(eng, np.vstack([base, rows]), 0, f"64 + {n} rows")


@pytest.mark.parametrize("metric,dims", [(0, 384), (1, 384), (0, 768)], ids=["cosine-384", "dot-384", "cosine-768"])
def test_an_append_from_inside_a_tile_over_more_than_4096_tiles(wax, metric, dims):
    """21 rows coded, 65 600 appended: the range begins inside tile 1 and touches tiles 1 .. 4 101, 4 101 tiles for 4 096 workgroups, so
    workgroups 0 .. 4 take a second tile, `tile0 + gridDim.x + blockIdx.x` with tile0 = 1 — the one term of the writer that no
    smaller append and no store written from row 0 exercises. The next query converts exactly the appended rows; the mirror then
    satisfies (a) row by row and equals a fresh engine's over the same rows bit for bit: codes, scale, err, the max-norm word, and
    the keys of three queries."""
    first, more = 21, 65_600
    rows, queries = R.corpus_for(metric, first + more, dims, seed=87), R.queries_for(dims)
    ids = np.arange(first + more, dtype=np.uint64)
    eng = wax.HIPVectorEngine(metric=wax.VectorMetric(metric), dimensions=dims)
    fresh = None
    try:
        eng.reserve(first + more)                                    # no new slab at the append: only the appended rows are converted
        eng.addBatch(ids[:first], rows[:first])
        eng.setTuning("mirror_bits", 8)
        warm(eng, queries[0])
        eng.addBatch(ids[first:], rows[first:])
        c = counters(eng)
        answer(eng, queries[0], 10, 2)
        d = delta(eng, c)
        assert (d["mirror8_conversions"], d["mirror8_rows_converted"], d["mirror8_passes"]) == (1, more, 1), d
        ctx = f"metric {metric} dims {dims}: {first} + {more} rows"
        check_mirror(eng, rows, metric, ctx)
        fresh = make_engine(wax, metric, dims, rows, ids)
        warm(fresh, queries[0])
        a, b = eng.mirror8Snapshot(), fresh.mirror8Snapshot()
        assert a[4] == b[4] == first + more
        assert np.array_equal(a[0], b[0]), f"{ctx}: codes, first difference at (row, element) {np.argwhere(a[0] != b[0])[0]}"
        for x, y, what in ((a[1], b[1], "scale"), (a[2], b[2], "err")):
            differ = np.flatnonzero(x.view(np.uint32) != y.view(np.uint32))
            assert differ.size == 0, f"{ctx}: {what} of {differ.size} rows, the first {differ[0]}"
        assert np.float32(a[3]).view(np.uint32) == np.float32(b[3]).view(np.uint32), f"{ctx}: max-norm word"
        for i, q in enumerate(queries[:3]):
            assert np.array_equal(eng.mirror8Keys(q).view(np.uint32), fresh.mirror8Keys(q).view(np.uint32)), f"{ctx}: keys of query {i}"
    finally:
        eng.close()
        if fresh is not None:
            fresh.close()


# ---- (b) the mirror after every kind of mutation --------------------------------------------------------------------------------

def test_mirror_follows_every_mutation(wax):
    """test_mutations_between_queries's sequence with a host model of the rows alongside: after the append the old rows are byte for
    byte what they were and the new ones satisfy (a); after every rebuild the whole mirror satisfies (a) against the model's rows in
    their new order and the max-norm word is tight again (the 1.5-norm upsert leaves with deserialize). Between a mutation — an append
    included — and the query that converts, the engine REFUSES the snapshot (the code mirror's fill is not current() from the mutation on), so it never
    hands out rows beyond, or other than, what was coded."""
    dims, k, n = 384, 10, 2005
    queries = R.queries_for(dims)
    rows = R.corpus_for(0, n, dims)
    model = OracleEngine(0, dims)
    model.addBatch(list(range(n)), rows)
    eng = make_engine(wax, 0, dims, rows)
    refused(wax, eng, "never built")
    warm(eng, queries[0])
    check_mirror(eng, model.matrix(), 0, "built")
    before = eng.mirror8Snapshot()

    new = np.stack([queries[1], queries[2]])
    eng.addBatch(np.array([900001, 900002], dtype=np.uint64), new)
    model.addBatch([900001, 900002], new)
    refused(wax, eng, "append")
    c = counters(eng)
    assert answer(eng, queries[1], k, 2)[0][0] == 900001
    d = delta(eng, c)
    assert (d["mirror8_conversions"], d["mirror8_rows_converted"], d["mirror8_passes"]) == (1, 2, 1), d
    after = eng.mirror8Snapshot()
    assert after[4] == eng.count == n + 2
    for a, b in zip(before[:3], after[:3]):
        assert np.array_equal(a.view(np.uint8), b[:n].view(np.uint8)), "append: the rows coded before it changed"
    R.check_rows(new, 0, after[0][n:], after[1][n:], after[2][n:], "appended rows")
    check_mirror(eng, model.matrix(), 0, "append")

    def stale_then_rebuilt(ctx):
        refused(wax, eng, ctx)
        c = counters(eng)
        for q in queries[:2]:                   # the next two take bf16 and leave the code mirror as it is
            answer(eng, q, k, 2)
            refused(wax, eng, ctx)
        answer(eng, queries[2], k, 2)           # the third rebuilds the whole code mirror
        d = delta(eng, c)
        assert (d["mirror8_passes"], d["mirror8_conversions"], d["mirror8_rows_converted"]) == (1, 1, model.count), (ctx, d)
        check_mirror(eng, model.matrix(), 0, ctx)

    up = (queries[3] * 1.5)[None, :]
    eng.addBatch(np.array([17], dtype=np.uint64), up)              # upsert of a coded row
    model.addBatch([17], up)
    stale_then_rebuilt("upsert")
    assert abs(eng.mirror8Snapshot(0, 0)[3] - 1.5) < 1e-4
    eng.remove(900001)
    model.remove(900001)
    stale_then_rebuilt("remove")
    assert eng.removeBatch([5, 900002, 1999, 123]) == 4
    for fid in (5, 900002, 1999, 123):
        model.remove(fid)
    stale_then_rebuilt("removeBatch")
    eng.reserve(eng.count * 4)                                      # a new store slab
    grown = R.corpus_for(0, 500, dims, seed=21)
    eng.addBatch(np.arange(10**6, 10**6 + 500, dtype=np.uint64), grown)
    model.addBatch(list(range(10**6, 10**6 + 500)), grown)
    stale_then_rebuilt("growth")
    other = make_engine(wax, 0, dims, R.corpus_for(0, 800, dims, seed=33))
    blob = other.serialize()
    eng.deserialize(blob)
    model.deserialize(blob)
    stale_then_rebuilt("deserialize")
    assert abs(eng.mirror8Snapshot(0, 0)[3] - 1.0) < 1e-4           # tight again: the row of norm 1.5 is gone


# ---- (c) a row whose quantisation error is aligned with the query -------------------------------------------------------------

@pytest.mark.parametrize("appended", [False, True], ids=["bulk", "appended"])
@pytest.mark.parametrize("metric", [0, 1], ids=["cosine", "dot"])
@pytest.mark.parametrize("dims", [384, 768])
def test_row_with_an_aligned_error_keeps_its_place(wax, dims, metric, appended):
    """The query is the row A itself. A's approximate distance is off by ~0.016 (384-d) — more than 200 honest neighbours lie nearer
    than that — and only its err (~0.074) makes it a candidate (test_mirror8_cpu.py: candidate 0 with err, not among the 64
    without, where the certificate would even pass). So A first, with the exact score, IS the test of err being measured over the
    whole row, stored, read and subtracted. Whether the query certifies follows the CPU model (these do not: the neighbours share A's
    large element and so its coarse scale)."""
    rows, a, at = R.aligned_store(dims, metric, appended)
    q = R.aligned_query(a, metric)
    eng = make_engine(wax, metric, dims, rows)
    warm(eng, R.queries_for(dims)[0])
    if appended:
        eng.addBatch(np.array([len(rows)], dtype=np.uint64), a[None, :])
        rows, at = np.vstack([rows, a[None, :]]), len(rows)
        c = counters(eng)
        answer(eng, R.queries_for(dims)[0], 10, 2)                   # converts the appended row, and nothing else
        assert delta(eng, c)["mirror8_rows_converted"] == 1
    coded = R.Coded(rows, metric)
    for k in (1, 5):
        ctx = f"{dims}-d metric {metric} appended {appended} k={k}"
        margin = coded.margin(q, k)
        got, certified = one_case(eng, q, k, ctx)
        print(f"{ctx}: margin {margin:.6f}, certified {certified}, first {got[0][0]} score {got[1][0]:.8f}")
        assert got[0][0] == at, f"{ctx}: the aligned row lost its place: {got[0]}"
        e_ids, e_scores, _, _ = oracle.search(metric, rows, None, q, k + 16)
        want = 1.0 if metric == 0 else float(e_scores[0])            # (dot: q.A less the convention's offset, from the f64 oracle)
        assert abs(float(got[1][0]) - want) <= 1e-6 * abs(want), (ctx, got[1][0], want)
        assert_parity(got[0], got[1], e_ids[:k], e_scores[:k], all_exp_scores=e_scores, ctx=ctx)
        assert certified == (margin > 0), f"{ctx}: certified {certified}, the model's margin is {margin}"
    check_mirror(eng, rows, metric, "aligned store")


# ---- (d) the certificate decision on a ladder -------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", [0, 1], ids=["cosine", "dot"])
@pytest.mark.parametrize("dims", [384, 768])
def test_certificate_decision_on_a_ladder(wax, dims, metric):
    """Rungs three slacks apart below the 64th key: margin(k) = lb_KP - slack - d_k changes sign inside k = 1 .. 16. For every query
    and k the device certifies exactly when the f64 model's margin is positive; cases with |margin| <= slack are left out (there the
    f32 key may differ from the f64 one by what mirror8_slack claims to bound — no other tolerance). That pins err, the bias, the
    byte order and lb_KP on the device to within one slack (~1.5e-4 at 384-d); a lost or halved err moves the key by 4e-3 to 8e-3.
    Four certified queries follow every case, so the breaker (8 uncertified of the last 32) never diverts one to bf16."""
    rows, queries = R.ladder_store(dims, metric)
    eng = make_engine(wax, metric, dims, rows)
    warm(eng, queries[0], k=1)
    coded = R.Coded(rows, metric)
    checked = wrong = 0
    for i, k, margin, sl in R.ladder_expectations(coded, queries):
        ctx = f"{dims}-d metric {metric} query {i} k={k} margin {margin / sl:+.2f} slacks"
        _, certified = one_case(eng, queries[i], k, ctx)
        print(f"{ctx}: certified {certified}")
        if abs(margin) > sl:
            checked += 1
            wrong += certified != (margin > 0)
            assert certified == (margin > 0), ctx
        for _ in range(4):
            assert one_case(eng, queries[i], 1, ctx + " (filler)")[1]
    assert eng.getTuning("mirror8_breaker_trips") == 0 and checked >= len(queries) * (R.MAX_K - 3) and wrong == 0


# ---- (e) row-count edges of the scan ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", [0, 1], ids=["cosine", "dot"])
@pytest.mark.parametrize("dims", [384, 768])
def test_scan_row_count_edges(wax, dims, metric):
    """1, 63, 64, 65 rows and one less, exactly, one more than two wave iterations (32 rows each at 384-d, 16 at 768-d), a lone
    query and a group of four: the f32 scan's answers; below 64 rows the 64th key is padding and every query is counted uncertified;
    from 64 rows on the certificate follows the model's margin."""
    queries = R.queries_for(dims, 4)
    ks = (1, 5, 10, 16)
    for n in R.scan_edge_counts(dims):
        rows = R.corpus_for(metric, n, dims, seed=81)
        coded = R.Coded(rows, metric)
        eng = make_engine(wax, metric, dims, rows)
        warm(eng, queries[0], k=1)
        ctx = f"{n} rows of {dims}, metric {metric}"
        got, certified = one_case(eng, queries[1], 5, ctx)
        assert len(got[0]) == min(5, n) and certified == (coded.margin(queries[1], min(5, n)) > 0), ctx
        eng.setTuning("scan_mirror", 0)
        f32 = [eng.searchArrays(q, k) for q, k in zip(queries, ks)]
        eng.setTuning("scan_mirror", 2)
        eng.setTuning("mirror_share", 2)
        c = counters(eng)
        tickets = [eng.submit(q, k) for q, k in zip(queries, ks)]
        group = [eng.collect(t, k) for t, k in zip(tickets, ks)]
        d = delta(eng, c)
        eng.setTuning("mirror_share", 1)
        assert all(same(a, b) for a, b in zip(group, f32)), ctx
        expected = sum(0 if coded.margin(q, min(k, n)) > 0 else 1 for q, k in zip(queries, ks))
        assert d["mirror8_passes"] >= 1 and d["mirror_scans"] == 4 and d["mirror8_unavailable"] == 0, (ctx, d)
        assert d["mirror8_fallbacks"] == expected and (n >= R.KP or expected == 4), (ctx, d, expected)
