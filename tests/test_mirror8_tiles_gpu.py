"""The 8-bit code mirror in tile order (wax_amd/csrc/mirror8_layout.h): the writer (mirror8_kernel), the reader
(code8_pass in every kernel that runs it) and the read-out (mirror8Snapshot, which hands out rows) must agree on where the code of
(row, element) sits, at every row count around a 16-row tile, for appends that begin inside a tile, in shared passes and under
row bitmaps. 384-d and 768-d, cosine and dot; stores are forced onto the code mirror as test_mirror8_gpu.py does it.

  tile edges     n in {1, 15, 16, 17, 31, 32, 33, 100}. Integer rows with one 127 and a different value at every element: their codes
                 ARE the rows in mirror8_ref's model (asserted), so the snapshot's codes must equal the model's byte for byte; for dot
                 the model's scale (exactly 1) too, with an err of one unit of the smallest f32. For cosine scale and err of every
                 row go through mirror8_ref.check_rows, the model's own bounds: the norm and err are sums in f32 on the device and in
                 f64 in the model, no bit pattern is common to both. Gaussian rows (n = 17, 100) go through check_rows as well.
                 Keys: test_mirror8_mfma_gpu.py's check, every key within 1e-6 (1 + ||q|| ||v||) of the f64 model made from the
                 snapshot's codes.
  element order  33 rows, the one-hot queries e_j for every j < D: the key of row r is then 1 - scale_r code_rj (/ 1) - err_r, so a
                 writer that puts element j where operand B expects another one shows on that j.
  appends        21 rows coded, 5 appended (rows 21 .. 25: inside tile 1, which already holds coded rows), a query, 40 more (tile 1
                 again, up into tile 4), a query: snapshot and keys of all rows equal a fresh engine's, bit for bit; the answers are the
                 f32 scan's. A pass over fewer than 64 rows cannot certify (the finish wants a 64th key) and every uncertified answer
                 feeds the "mirror_bits" breaker, so at 26 rows three queries are asked and may fall back; from 64 rows on all eight
                 are, with "mirror8_fallbacks" 0: at 66 rows, and at every step of the same sequence behind 64 rows that were there
                 from the start (90 and 130 rows).
  groups, masks  n = 33 and n = 4 099: four parked queries answer as alone; a predicate ticket that passes only rows 16 .. 31 and one
                 that passes only row n - 1 answer as the blocking predicate search, alone and parked with two unfiltered tickets.
"""
import numpy as np
import pytest

import mirror8_planes_ref as P
import mirror8_ref as R8

EDGES = [1, 15, 16, 17, 31, 32, 33, 100]


@pytest.fixture(scope="module")
def wax(hip_lib):
    import wax_amd
    if hip_lib.wax_hip_device_count() == 0:
        pytest.skip("no HIP device on this host: the gpu-marked tests run on the MI355X box (pytest -m gpu)")
    assert hip_lib.wax_hip_available() == 1, "a HIP device is visible but it is not gfx950: the HIP path needs an MI355X"
    return wax_amd


def integer_rows(n, dims, seed=5):
    """Integers in [-126, 126], dense and different from row to row, and one 127 per row at a place that moves with the row."""
    rng = np.random.default_rng(seed + dims)
    x = rng.integers(-126, 127, size=(n, dims)).astype(np.float32)
    x[np.arange(n), (7 * np.arange(n) + 3) % dims] = 127.0
    return x


def gaussian_rows(metric, n, dims, seed=0):
    return R8.corpus_for(metric, n, dims, seed=seed)


def ids_of(first, n):
    return np.arange(first, first + n, dtype=np.uint64) * 3 + 7


def force_code_mirror(eng):
    for key, value in (("scan_mirror", 2), ("mirror_share", 0), ("mirror_bits", 8)):
        eng.setTuning(key, value)


def build_code_mirror(eng, q):
    """A missing code mirror is built by the third eligible query in a row."""
    c0 = eng.getTuning("mirror8_conversions")
    for _ in range(3):
        eng.searchArrays(q, 1)
    assert eng.getTuning("mirror8_conversions") - c0 == 1


def coded_engine(wax, metric, rows, q, reserve=None):
    eng = wax.HIPVectorEngine(metric=wax.VectorMetric(metric), dimensions=rows.shape[1])
    if reserve:
        eng.reserve(reserve)
    eng.addBatch(ids_of(0, len(rows)), rows)
    force_code_mirror(eng)
    build_code_mirror(eng, q)
    return eng


def check_keys(eng, rows, q, metric, ctx):
    """test_mirror8_mfma_gpu.py's Gaussian check: every key within 1e-6 (1 + ||q|| ||v||) of the f64 model of the quantised form, made
    from the codes, scale and err that the snapshot hands out."""
    codes_u8, scale, err, _, coded = eng.mirror8Snapshot()
    n = len(rows)
    assert coded == n and codes_u8.shape == rows.shape
    keys = eng.mirror8Keys(q).astype(np.float64)
    assert keys.shape == (n,)
    model = P.keys64(q, codes_u8.astype(np.int64) - 128, scale, err, metric)
    qn = float(np.linalg.norm(q.astype(np.float64)))
    both = qn * np.linalg.norm(rows.astype(np.float64), axis=1) if metric == 1 else np.ones(n)
    gap = np.abs(keys - model)
    worst = int(np.argmax(gap / (1.0 + both)))
    assert np.all(gap <= 1e-6 * (1.0 + both)), f"{ctx}: row {worst} key {keys[worst]} model {model[worst]}"
    return float(np.max(gap / (1.0 + both)))


@pytest.mark.gpu
@pytest.mark.parametrize("metric,dims", P.CASES, ids=P.CASE_IDS)
def test_tile_edges_codes_and_keys(wax, metric, dims):
    qs = P.queries(dims)
    for n in EDGES:
        rows = integer_rows(n, dims)
        want_codes, want_scale, _ = R8.quantise(R8.normalise(rows, metric))
        assert np.array_equal(want_codes, rows.astype(np.int16)), "the model's codes of these rows are the rows"
        eng = coded_engine(wax, metric, rows, qs[0])
        try:
            codes_u8, scale, err, max_norm, coded = eng.mirror8Snapshot()
            ctx = f"metric {metric} dims {dims} n {n}"
            assert coded == n
            bad = np.argwhere(codes_u8 != R8.to_bytes(want_codes))
            assert bad.size == 0, f"{ctx}: {len(bad)} codes differ from the model, first at (row, element) {bad[0]}"
            if metric == 1:      # coded without error: err is one unit of the smallest f32 in units of 2^ex, as test_mirror8_mfma_gpu.py has it
                assert np.array_equal(scale, want_scale) and np.all(scale == 1.0) and np.all(err < 1e-40) and np.all(err > 0), f"{ctx}: scale, err"
            else:
                R8.check_rows(rows, metric, codes_u8, scale, err, ctx)
            R8.check_max_norm(rows, max_norm, ctx)
            # a part of the read-out that begins and ends inside tiles
            if n >= 17:
                part = eng.mirror8Snapshot(3, n - 4)
                assert np.array_equal(part[0], codes_u8[3:n - 1]) and np.array_equal(part[1], scale[3:n - 1]) and np.array_equal(part[2], err[3:n - 1]), ctx
            worst = max(check_keys(eng, rows, q, metric, f"{ctx} query {i}") for i, q in enumerate(qs[:3]))
            print(f"{ctx}: largest |key - model| / (1 + ||q|| ||v||) = {worst:.3e}")
        finally:
            eng.close()
    for n in (17, 100):
        rows = gaussian_rows(metric, n, dims, seed=3)
        eng = coded_engine(wax, metric, rows, qs[0])
        try:
            codes_u8, scale, err, max_norm, _ = eng.mirror8Snapshot()
            ctx = f"gaussian metric {metric} dims {dims} n {n}"
            R8.check_rows(rows, metric, codes_u8, scale, err, ctx)
            R8.check_max_norm(rows, max_norm, ctx)
            for i, q in enumerate(qs[:3]):
                check_keys(eng, rows, q, metric, f"{ctx} query {i}")
        finally:
            eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("metric,dims", P.CASES, ids=P.CASE_IDS)
def test_every_element_sits_where_operand_b_expects_it(wax, metric, dims):
    n = 33
    rows = gaussian_rows(metric, n, dims, seed=9)
    eng = coded_engine(wax, metric, rows, P.queries(dims)[0])
    try:
        codes_u8, scale, err, _, _ = eng.mirror8Snapshot()
        codes = codes_u8.astype(np.int64) - 128
        both = np.linalg.norm(rows.astype(np.float64), axis=1) if metric == 1 else np.ones(n)
        worst = 0.0
        for j in range(dims):
            q = np.zeros(dims, dtype=np.float32)
            q[j] = 1.0
            keys = eng.mirror8Keys(q).astype(np.float64)
            model = P.keys64(q, codes, scale, err, metric)
            gap = np.abs(keys - model) / (1.0 + both)
            worst = max(worst, float(gap.max()))
            assert np.all(gap <= 1e-6), f"metric {metric} dims {dims}: element {j}, row {int(np.argmax(gap))}: key {keys[np.argmax(gap)]} model {model[np.argmax(gap)]}"
        # the check has teeth: a neighbouring element's code moves some row's key by far more than the tolerance
        step = np.abs(np.diff(codes, axis=1)).max(axis=0) * scale.astype(np.float64).min()
        assert np.all(step > 100 * 1e-6 * (1.0 + both.max())), "two neighbouring elements have the same codes in every row"
        print(f"metric {metric} dims {dims}: largest |key - model| / (1 + ||q|| ||v||) over {dims} one-hot queries = {worst:.3e}")
    finally:
        eng.close()


def exact_answers(eng, qs, k):
    eng.setTuning("scan_mirror", 0)
    out = [eng.searchArrays(q, k) for q in qs]
    eng.setTuning("scan_mirror", 2)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("prefix", [0, 64], ids=["from-row-0", "behind-64-rows"])
@pytest.mark.parametrize("metric,dims", P.CASES, ids=P.CASE_IDS)
def test_appends_that_start_inside_a_tile(wax, metric, dims, prefix):
    total = prefix + 21 + 5 + 40
    rows, qs = gaussian_rows(metric, total, dims, seed=13), P.queries(dims)
    eng = wax.HIPVectorEngine(metric=wax.VectorMetric(metric), dimensions=dims)
    try:
        eng.reserve(total)                                           # no new slab at the appends: only the appended rows are converted
        count = prefix + 21
        eng.addBatch(ids_of(0, count), rows[:count])
        force_code_mirror(eng)
        build_code_mirror(eng, qs[0])
        for more in (5, 40):
            eng.addBatch(ids_of(count, more), rows[count:count + more])
            count += more
            ctx = f"metric {metric} dims {dims}: {count} rows after an append of {more}"
            exact = exact_answers(eng, qs, 10)
            c0 = {key: eng.getTuning(key) for key in ("mirror8_conversions", "mirror8_rows_converted", "mirror8_fallbacks", "mirror8_passes")}
            # the first one converts the appended rows, and nothing else. Below 64 rows every answer is an uncertified one and feeds the
            # "mirror_bits" breaker (8 of the last 32 close the 8-bit route): three queries there, all eight from 64 rows on
            asked = qs if count >= R8.KP else qs[:3]
            got = [eng.searchArrays(q, 10) for q in asked]
            d = {key: eng.getTuning(key) - c0[key] for key in c0}
            assert (d["mirror8_conversions"], d["mirror8_rows_converted"], d["mirror8_passes"]) == (1, more, len(asked)), f"{ctx}: {d}"
            for i, (g, w) in enumerate(zip(got, exact)):
                assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]), f"{ctx}: query {i}"
            if count >= R8.KP:
                assert d["mirror8_fallbacks"] == 0, f"{ctx}: {d}"
            fresh = coded_engine(wax, metric, rows[:count], qs[0])
            try:
                a, b = eng.mirror8Snapshot(), fresh.mirror8Snapshot()
                assert a[4] == b[4] == count
                assert np.array_equal(a[0], b[0]), f"{ctx}: codes, first difference at (row, element) {np.argwhere(a[0] != b[0])[0]}"
                assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32)), f"{ctx}: scale / err"
                assert np.float32(a[3]).view(np.uint32) == np.float32(b[3]).view(np.uint32), f"{ctx}: max-norm word"
                for i, q in enumerate(qs[:3]):
                    assert np.array_equal(eng.mirror8Keys(q).view(np.uint32), fresh.mirror8Keys(q).view(np.uint32)), f"{ctx}: keys of query {i}"
            finally:
                fresh.close()
    finally:
        eng.close()


def same(got, want, ctx):
    assert np.array_equal(got[0], want[0]), f"{ctx}: ids {got[0]} != {want[0]}"
    assert np.array_equal(got[1], want[1]), f"{ctx}: scores differ"


def attributed_engine(wax, metric, rows, q):
    """Coded, with ts = row and no flags, predicate tickets on the masked 8-bit pass."""
    n = len(rows)
    eng = wax.HIPVectorEngine(metric=wax.VectorMetric(metric), dimensions=rows.shape[1])
    eng.addBatch(ids_of(0, n), rows)
    assert eng.setAttributes(ids_of(0, n), np.arange(n, dtype=np.int64), np.zeros(n, dtype=np.uint32)) == n
    eng.setTuning("predicate_mirror", 2)
    force_code_mirror(eng)
    build_code_mirror(eng, q)
    return eng


# Two engines per store: an uncertified unfiltered answer feeds the "mirror_bits" breaker (8 of the last 32 close the 8-bit route),
# and at 33 rows no pass certifies — the nine of the first test would leave the second one nothing to ride.

@pytest.mark.gpu
@pytest.mark.parametrize("n", [33, 4099])
@pytest.mark.parametrize("metric,dims", P.CASES, ids=P.CASE_IDS)
def test_four_parked_queries_answer_as_alone(wax, metric, dims, n):
    rows, qs = gaussian_rows(metric, n, dims, seed=17), P.queries(dims)
    k = 10
    eng = coded_engine(wax, metric, rows, qs[0])
    try:
        alone = [eng.searchArrays(q, k) for q in qs[:4]]
        eng.setTuning("mirror_share", 2)
        p8, shared = eng.getTuning("mirror8_passes"), eng.getTuning("mirror_shared_queries")
        tickets = [eng.submit(q, k) for q in qs[:4]]
        got = [eng.collect(t, k) for t in tickets]
        assert eng.getTuning("mirror8_passes") - p8 == 1 and eng.getTuning("mirror_shared_queries") - shared == 4, "one pass of four"
        for i in range(4):
            same(got[i], alone[i], f"metric {metric} dims {dims} n {n}: query {i} in a pass of four")
        if n >= R8.KP:
            assert eng.getTuning("mirror8_fallbacks") == 0
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [33, 4099])
@pytest.mark.parametrize("metric,dims", P.CASES, ids=P.CASE_IDS)
def test_tickets_under_a_tile_and_a_tail_bitmap_answer_as_the_blocking_search(wax, metric, dims, n):
    rows, qs = gaussian_rows(metric, n, dims, seed=17), P.queries(dims)
    k, ids = 10, ids_of(0, n)
    eng = attributed_engine(wax, metric, rows, qs[0])
    try:
        eng.setTuning("mirror_share", 2)
        ctx = f"metric {metric} dims {dims} n {n}"
        free = exact_answers(eng, [qs[0], qs[3]], k)
        tile1, last = {"timeRange": (16, 32)}, {"timeRange": (n - 1, None)}
        want1, want_last = eng.searchFiltered(qs[1], k, **tile1), eng.searchFiltered(qs[2], k, **last)
        assert len(want1[0]) == k and set(want1[0]) <= set(ids[16:32]) and list(want_last[0]) == [ids[n - 1]]
        same(eng.collect(eng.submitFiltered(qs[1], k, **tile1), k), want1, f"{ctx}: rows 16 .. 31, alone")
        same(eng.collect(eng.submitFiltered(qs[2], k, **last), k), want_last, f"{ctx}: row n - 1, alone")
        tickets = [eng.submit(qs[0], k), eng.submitFiltered(qs[1], k, **tile1), eng.submitFiltered(qs[2], k, **last), eng.submit(qs[3], k)]
        got = [eng.collect(t, k) for t in tickets]
        same(got[0], free[0], f"{ctx}: unfiltered member 0 of a mixed set")
        same(got[1], want1, f"{ctx}: rows 16 .. 31 in a mixed set")
        same(got[2], want_last, f"{ctx}: row n - 1 in a mixed set")
        same(got[3], free[1], f"{ctx}: unfiltered member 3 of a mixed set")
    finally:
        eng.close()
