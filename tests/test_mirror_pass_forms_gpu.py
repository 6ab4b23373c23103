"""Every form of the pass over a compressed mirror (mirror_pass.h) gives one query one answer: alone, as a member of a shared pass of
2, 3 or 4, under a row bitmap that every row passes (bf16), and again alone and shared on the 8-bit code mirror — each time the
hits (ids and scores) of the exact f32 scan of the same engine, bit for bit, with the counters of the intended form and no fallback.

The store has 1003 rows: no multiple of any form's rows per wave iteration (16 / 8 on bf16, 32 / 16 on 8 bits at 384-d / 768-d), so the
last chunk clamps; "grid_blocks" 2 (what "scan_grid" then reports for these rows) makes every wave run several iterations. Zero
fallbacks are a condition, not a hope: test_the_seeded_data_certifies_in_every_form shows on the CPU, with the float64 models of
predicate_mirror_ref.py and mirror8_ref.py, that every (store, query) certifies with a margin far above the kernels' f32 summation
error. A bitmap of all rows leaves the bf16 certificate as it is without one, so one model serves the lone, shared and masked forms."""
import functools

import numpy as np
import pytest

import mirror8_ref as R8
import oracle
import predicate_mirror_ref as R16

N, K, N_QUERIES, STORE_SEED, QUERY_SEED = 1003, 10, 8, 20261019, 11
GRID = 2
CASES = [(m, d) for m in (0, 1) for d in (384, 768)]
CASE_IDS = [f"{'cosine' if m == 0 else 'dot'}-{d}" for m, d in CASES]
PASS_ALL_BIT = 1 << 9                # a flag no row carries: denying it passes every row

C16 = ("mirror_scans", "mirror_passes", "mirror_shared_passes", "mirror_shared_queries", "mirror8_passes")
ZERO = ("mirror_scan_fallbacks", "mirror_scan_unavailable", "mirror8_fallbacks", "mirror8_unavailable", "mirror8_breaker_trips",
        "predicate_mirror_fallbacks", "predicate_mirror_unavailable")
PREDICATE = ("predicate_searches", "predicate_gather_searches", "predicate_masked_scans", "predicate_mirror_scans")


@functools.lru_cache(maxsize=None)
def store_rows(metric, dims):
    x = oracle.gaussian_unit_rows(0, N, dims, seed=STORE_SEED)
    if metric == 1:                  # dot: rows of norms 0.5 .. 2
        x = x * np.random.default_rng(STORE_SEED + 7).uniform(0.5, 2.0, size=(N, 1)).astype(np.float32)
    return np.ascontiguousarray(x, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def queries(dims):
    return oracle.gaussian_unit_queries(N_QUERIES, dims, seed=QUERY_SEED)


@pytest.mark.parametrize("metric,dims", CASES, ids=CASE_IDS)
def test_the_seeded_data_certifies_in_every_form(metric, dims):
    rows, qs = store_rows(metric, dims), queries(dims)
    everything = np.ones(N, dtype=bool)
    m16 = R16.Model(metric, rows, qs)
    bf16 = [m16.margin(everything, i, K) for i in range(N_QUERIES)]
    coded = R8.Coded(rows, metric)
    code8 = [coded.margin(q, K) for q in qs]
    print(f"metric {metric} dims {dims}: smallest margin bf16 {min(bf16):.5f}, 8 bits {min(code8):.5f}")
    # the floor of predicate_mirror_ref.py: both sides' f32 summation errors (3 D 2^-24 each, twice that for norms <= 2) stay below it
    assert min(bf16) > R16.MARGIN_FLOOR and min(code8) > R16.MARGIN_FLOOR


@pytest.fixture(scope="module")
def wax(hip_lib):
    import wax_amd
    if hip_lib.wax_hip_device_count() == 0:
        pytest.skip("no HIP device on this host: the gpu-marked tests run on the MI355X box (pytest -m gpu)")
    assert hip_lib.wax_hip_available() == 1, "a HIP device is visible but it is not gfx950: the HIP path needs an MI355X"
    return wax_amd


@pytest.fixture(scope="module", params=CASES, ids=CASE_IDS)
def store(request, wax):
    """(engine, queries, the exact f32 answers): mirrors off for the reference, computed once."""
    metric, dims = request.param
    ids = np.arange(N, dtype=np.uint64) * 3 + 7
    eng = wax.HIPVectorEngine(metric=wax.VectorMetric(metric), dimensions=dims)
    eng.addBatch(ids, store_rows(metric, dims))
    assert eng.setAttributes(ids, np.arange(N, dtype=np.int64), np.zeros(N, dtype=np.uint32)) == N
    eng.setTuning("grid_blocks", GRID)
    assert eng.getTuning("scan_grid") == GRID
    eng.setTuning("scan_mirror", 0)
    eng.setTuning("mirror_share", 0)
    qs = queries(dims)
    exact = [eng.searchArrays(q, K) for q in qs]
    assert all(len(e[0]) == K for e in exact)
    yield eng, qs, exact
    eng.close()


def snapshot(eng, names):
    return [eng.getTuning(n) for n in names]


def assert_same(got, want, ctx):
    assert np.array_equal(got[0], want[0]), f"{ctx}: ids differ from the exact f32 scan"
    assert np.array_equal(got[1], want[1]), f"{ctx}: scores differ from the exact f32 scan"


def lone_and_shared(eng, qs, exact, bits):
    """Every query alone, then as the first member of passes of 2, 3 and 4 (the others follow it in the list)."""
    on8 = 1 if bits == 8 else 0
    eng.setTuning("scan_mirror", 2)
    for i, q in enumerate(qs):
        eng.setTuning("mirror_share", 0)
        before = snapshot(eng, C16)
        assert_same(eng.searchArrays(q, K), exact[i], f"{bits} bits, query {i} alone")
        assert [a - b for a, b in zip(snapshot(eng, C16), before)] == [1, 1, 0, 0, on8], f"{bits} bits, query {i} alone"
        eng.setTuning("mirror_share", 2)
        for g in (2, 3, 4):
            members = [(i + j) % N_QUERIES for j in range(g)]
            before = snapshot(eng, C16)
            tickets = [eng.submit(qs[m], K) for m in members]
            got = [eng.collect(t, K) for t in tickets]
            assert [a - b for a, b in zip(snapshot(eng, C16), before)] == [g, 1, 1, g, on8], f"{bits} bits, query {i} in a pass of {g}"
            for m, hits in zip(members, got):
                assert_same(hits, exact[m], f"{bits} bits, query {m} in a pass of {g} behind query {i}")
    eng.setTuning("mirror_share", 0)
    eng.setTuning("scan_mirror", 0)


@pytest.mark.gpu
def test_every_form_answers_as_the_exact_scan(store):
    eng, qs, exact = store
    zero = snapshot(eng, ZERO)

    eng.setTuning("mirror_bits", 16)
    lone_and_shared(eng, qs, exact, 16)

    # bf16 under a bitmap that every row passes
    eng.setTuning("predicate_route", 2)
    eng.setTuning("predicate_mirror", 2)
    for i, q in enumerate(qs):
        before = snapshot(eng, PREDICATE)
        assert_same(eng.searchFiltered(q, K, denyFlags=PASS_ALL_BIT), exact[i], f"query {i} under the bitmap")
        assert [a - b for a, b in zip(snapshot(eng, PREDICATE), before)] == [1, 0, 1, 1], f"query {i} under the bitmap"
    eng.setTuning("predicate_route", 0)
    eng.setTuning("predicate_mirror", 1)

    # the code mirror is built by the third eligible query in a row (the first two take bf16)
    eng.setTuning("mirror_bits", 8)
    eng.setTuning("scan_mirror", 2)
    c0 = eng.getTuning("mirror8_conversions")
    for _ in range(3):
        eng.searchArrays(qs[0], K)
    assert eng.getTuning("mirror8_conversions") - c0 == 1 and eng.getTuning("mirror8_rows_converted") >= N
    lone_and_shared(eng, qs, exact, 8)

    assert snapshot(eng, ZERO) == zero, dict(zip(ZERO, snapshot(eng, ZERO)))
