"""The 8-bit pass on the matrix pipe, row by row, through `mirror8Keys` (the key the lone scan computes for every row, by the scan's
own body) and `mirror8Snapshot` (the codes, scale and err those keys were made from):

  layout      integer rows and an integer query (mirror8_planes_ref.layout_*): delta is exactly 1 and every sum fits 24 bits, so for
              dot (scale exactly 1, err ~1e-45) the key is 1 - S exactly and S must equal the int64 dot — a wrong lane map of either
              MFMA operand, a k permutation that A and B do not share, or a swap of rows and columns changes it; for cosine S is
              recovered from the key to within the epilogue's roundings;
  Gaussian    every key within 1e-6 (1 + ||q|| ||v||) of the f64 model of the quantised form, and no key above the row's exact
              distance + slack (the lower-bound property);
  refusal     no keys from a mirror that is not valid;
  end to end  alone and in passes of 2, 3 and 4 with mixed k in 1 .. 16: the exact f32 scan's hits bit for bit, no fallback
              (test_mirror8_planes_cpu.py shows that every (store, query, k) used here certifies with margin).

1 003 rows with "grid_blocks" 2 (no multiple of the 16-row tile or of a wave iteration: the last tile clamps, every wave runs several
iterations) and a 15-row store (less than one tile)."""
import numpy as np
import pytest

import mirror8_planes_ref as P
import mirror8_ref as R8

GRID = 2
ZERO = ("mirror8_fallbacks", "mirror8_unavailable", "mirror8_breaker_trips", "mirror_scan_fallbacks", "mirror_scan_unavailable")


@pytest.fixture(scope="module")
def wax(hip_lib):
    import wax_amd
    if hip_lib.wax_hip_device_count() == 0:
        pytest.skip("no HIP device on this host: the gpu-marked tests run on the MI355X box (pytest -m gpu)")
    assert hip_lib.wax_hip_available() == 1, "a HIP device is visible but it is not gfx950: the HIP path needs an MI355X"
    return wax_amd


def coded_engine(wax, metric, rows, first_query):
    """An engine over `rows` whose code mirror is valid: built by the third eligible query in a row."""
    n, dims = rows.shape
    eng = wax.HIPVectorEngine(metric=wax.VectorMetric(metric), dimensions=dims)
    eng.addBatch(np.arange(n, dtype=np.uint64) * 3 + 7, rows)
    eng.setTuning("grid_blocks", GRID)
    eng.setTuning("scan_mirror", 2)
    eng.setTuning("mirror_share", 0)
    eng.setTuning("mirror_bits", 8)
    c0 = eng.getTuning("mirror8_conversions")
    for _ in range(3):
        eng.searchArrays(first_query, 1)
    assert eng.getTuning("mirror8_conversions") - c0 == 1
    return eng


def device_model(eng, n):
    codes_u8, scale, err, max_norm, coded = eng.mirror8Snapshot()
    assert coded == n and codes_u8.shape[0] == n
    return codes_u8.astype(np.int64) - 128, scale, err, max_norm


@pytest.mark.gpu
@pytest.mark.parametrize("n", [P.N, P.SMALL_N], ids=["1003-rows", "15-rows"])
@pytest.mark.parametrize("metric,dims", P.CASES, ids=P.CASE_IDS)
def test_the_integer_sum_of_every_row_is_exact(wax, metric, dims, n):
    rows, q = P.layout_store(n, dims), P.layout_query(dims)
    eng = coded_engine(wax, metric, rows, q)
    try:
        codes, scale, err, _ = device_model(eng, n)
        assert np.array_equal(codes, rows.astype(np.int64)), "the codes of integer rows with a 127 are the rows"
        m, delta = P.quantise(q)
        assert delta == 1.0
        S = P.integer_sums(codes, m)
        keys = eng.mirror8Keys(q).astype(np.float64)
        assert keys.shape == (n,)
        qn = float(np.linalg.norm(q.astype(np.float64)))
        if metric == 1:
            assert np.all(scale == 1.0) and np.all(err < 1e-40)
            got = 1.0 - keys                                     # exact: |S| < 2^24, and ||q|| err is below half an ulp of 1 - S
            bad = np.flatnonzero(got != S)
            assert bad.size == 0, f"{bad.size} rows differ from the int64 dot, first row {bad[0]}: {got[bad[0]]} != {S[bad[0]]}"
        else:
            # key = fl(fl(1 - fl(fl(scale) S) / ||q||) - err): four roundings of values <= 2 + the f32 reciprocal of ||q||
            unit = scale.astype(np.float64) / qn                  # what one unit of S moves the key by
            got = (1.0 - keys - err.astype(np.float64)) / unit
            tol = 6.0 * 2.0 ** -24 * (2.0 + np.abs(S) * unit) / unit
            bad = np.flatnonzero(np.abs(got - S) > tol)
            print(f"cosine {dims} n {n}: largest |S recovered - S| / tolerance {np.max(np.abs(got - S) / tol):.3f}, tolerance in units of S {tol.max():.3f}")
            assert bad.size == 0, f"{bad.size} rows differ, first row {bad[0]}: {got[bad[0]]} against {S[bad[0]]} +- {tol[bad[0]]}"
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [P.N, P.SMALL_N], ids=["1003-rows", "15-rows"])
@pytest.mark.parametrize("metric,dims", P.CASES, ids=P.CASE_IDS)
def test_gaussian_keys_follow_the_model_and_bound_the_distance(wax, metric, dims, n):
    rows, qs = P.store_rows(metric, dims)[:n], P.queries(dims)
    eng = coded_engine(wax, metric, rows, qs[0])
    try:
        codes, scale, err, max_norm = device_model(eng, n)
        vnorm = np.linalg.norm(rows.astype(np.float64), axis=1)
        for i, q in enumerate(list(qs[:3]) + [3.0 * qs[3]]):         # (a query of norm 3: the dot key scales, the cosine key does not)
            qn = float(np.linalg.norm(q.astype(np.float64)))
            keys = eng.mirror8Keys(q).astype(np.float64)
            model = P.keys64(q, codes, scale, err, metric)
            both = qn * vnorm if metric == 1 else np.ones(n)
            gap = np.abs(keys - model)
            print(f"metric {metric} dims {dims} n {n} query {i}: largest |key - model| / (1 + ||q|| ||v||) = {np.max(gap / (1.0 + both)):.3e}")
            assert np.all(gap <= 1e-6 * (1.0 + both)), f"query {i}: row {int(np.argmax(gap))} key {keys[np.argmax(gap)]} model {model[np.argmax(gap)]}"
            exact = R8.exact_distances(rows, q, metric)
            over = keys - exact - R8.slack(dims, metric, qn, max_norm)
            assert np.all(over <= 0), f"query {i}: the key of row {int(np.argmax(over))} is no lower bound: {over.max()} above distance + slack"
    finally:
        eng.close()


@pytest.mark.gpu
def test_keys_of_a_mirror_that_is_not_valid_are_refused(wax):
    rows, qs = P.store_rows(0, 384), P.queries(384)
    eng = wax.HIPVectorEngine(metric=wax.VectorMetric(0), dimensions=384)
    try:
        eng.addBatch(np.arange(P.N, dtype=np.uint64), rows)
        with pytest.raises(wax.EncodingError, match="code mirror is absent or not valid"):
            eng.mirror8Keys(qs[0])                               # never built
        eng.setTuning("scan_mirror", 2)
        eng.setTuning("mirror_bits", 8)
        for _ in range(3):
            eng.searchArrays(qs[0], 1)
        conversions = eng.getTuning("mirror8_conversions")
        assert eng.mirror8Keys(qs[0]).shape == (P.N,)
        assert eng.getTuning("mirror8_conversions") == conversions and eng.getTuning("mirror8_passes") >= 1
        passes = eng.getTuning("mirror8_passes")
        eng.mirror8Keys(qs[1])
        assert eng.getTuning("mirror8_passes") == passes        # no counter moves
        eng.addBatch(np.arange(P.N, P.N + 1, dtype=np.uint64), rows[:1])
        with pytest.raises(wax.EncodingError, match="code mirror is absent or not valid"):
            eng.mirror8Keys(qs[0])                               # stale after a mutation; not rebuilt here
        assert eng.getTuning("mirror8_conversions") == conversions
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("metric,dims", P.CASES, ids=P.CASE_IDS)
def test_alone_and_shared_with_mixed_k_answer_as_the_exact_scan(wax, metric, dims):
    rows, qs = P.store_rows(metric, dims), P.queries(dims)
    eng = wax.HIPVectorEngine(metric=wax.VectorMetric(metric), dimensions=dims)
    try:
        eng.addBatch(np.arange(P.N, dtype=np.uint64) * 3 + 7, rows)
        eng.setTuning("grid_blocks", GRID)
        eng.setTuning("scan_mirror", 0)
        eng.setTuning("mirror_share", 0)
        ks = sorted({1, R8.MAX_K} | {P.mixed_k(i) for i in range(P.N_QUERIES)})
        exact = {(i, k): eng.searchArrays(q, k) for i, q in enumerate(qs) for k in ks}
        eng.setTuning("mirror_bits", 8)
        eng.setTuning("scan_mirror", 2)
        for _ in range(3):
            eng.searchArrays(qs[0], 1)
        zero = [eng.getTuning(name) for name in ZERO]

        def same(got, i, k, ctx):
            want = exact[(i, k)]
            assert len(got[0]) == k and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), f"{ctx}: query {i}, k {k}"

        for i, q in enumerate(qs):
            eng.setTuning("mirror_share", 0)
            for k in (1, P.mixed_k(i), R8.MAX_K):
                p8 = eng.getTuning("mirror8_passes")
                same(eng.searchArrays(q, k), i, k, "alone")
                assert eng.getTuning("mirror8_passes") - p8 == 1
            eng.setTuning("mirror_share", 2)
            for g in (2, 3, 4):
                members = [(i + j) % P.N_QUERIES for j in range(g)]
                kk = [P.mixed_k(m) if j else (1, P.mixed_k(i), R8.MAX_K)[g - 2] for j, m in enumerate(members)]
                p8, shared = eng.getTuning("mirror8_passes"), eng.getTuning("mirror_shared_queries")
                tickets = [eng.submit(qs[m], k) for m, k in zip(members, kk)]
                got = [eng.collect(t, k) for t, k in zip(tickets, kk)]
                assert eng.getTuning("mirror8_passes") - p8 == 1 and eng.getTuning("mirror_shared_queries") - shared == g, f"a pass of {g}"
                for m, k, hits in zip(members, kk, got):
                    same(hits, m, k, f"a pass of {g} behind query {i}")
        assert [eng.getTuning(name) for name in ZERO] == zero, dict(zip(ZERO, [eng.getTuning(name) for name in ZERO]))
    finally:
        eng.close()
