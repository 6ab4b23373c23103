"""Single queries on the 8-bit code mirror ("mirror_bits" 8 under "scan_mirror" 2): the answer is the f32 scan's, bit for bit, whether
the per-row certificate held or failed; the counters say which mirror ran; mutations keep it so. The stores, the queries and the proof
that the Gaussian ones certify (and the duplicate / clustered ones cannot) are in mirror8_ref.py and test_mirror8_cpu.py.

A stale or missing code mirror is rebuilt by the third eligible query in a row since the last mutation (the first two take bf16):
`warm` spends those three."""
import numpy as np
import pytest

import mirror8_ref as R

pytestmark = pytest.mark.gpu

C8 = ("mirror8_passes", "mirror8_fallbacks", "mirror8_unavailable", "mirror8_conversions", "mirror8_rows_converted",
      "mirror8_breaker_trips", "mirror_scans", "mirror_passes", "mirror_scan_fallbacks", "mirror_shared_passes", "mirror_rows_converted")


@pytest.fixture(scope="module")
def wax(hip_lib):
    import wax_amd
    if hip_lib.wax_hip_device_count() == 0:
        pytest.skip("no HIP device on this host: the gpu-marked tests run on the MI355X box (pytest -m gpu)")
    assert hip_lib.wax_hip_available() == 1, "a HIP device is visible but it is not gfx950: the HIP path needs an MI355X"
    return wax_amd


def make_engine(wax, metric, dims, corpus, ids=None, bits=8, **kw):
    eng = wax.HIPVectorEngine(metric=wax.VectorMetric(metric), dimensions=dims, **kw)
    eng.addBatch(np.arange(len(corpus), dtype=np.uint64) if ids is None else ids, corpus)
    eng.setTuning("mirror_bits", bits)
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


def assert_same(eng, queries, k, ctx):
    for i, q in enumerate(queries):
        assert same(answer(eng, q, k, 2), answer(eng, q, k, 0)), f"{ctx}: query {i}, k={k}"


def run_group(eng, queries, ks, mirror, share):
    eng.setTuning("scan_mirror", mirror)
    eng.setTuning("mirror_share", share)
    tickets = [eng.submit(q, k) for q, k in zip(queries, ks)]
    return [eng.collect(t, k) for t, k in zip(tickets, ks)]


@pytest.fixture(scope="module", params=[(m, s) for m in (0, 1) for s in R.GAUSSIAN_SHAPES],
                ids=lambda p: f"{'cosine' if p[0] == 0 else 'dot'}-{p[1][0]}x{p[1][1]}")
def gaussian(request, wax):
    """One engine per (metric, shape), its code mirror built, shared by the tests below."""
    metric, (n, dims) = request.param
    eng = make_engine(wax, metric, dims, R.corpus_for(metric, n, dims))
    queries = R.queries_for(dims)
    d = warm(eng, queries[0])
    assert d["mirror8_rows_converted"] == n
    return eng, queries, n, dims


def test_lone_queries_equal_the_f32_scan_and_count(gaussian):
    eng, queries, n, dims = gaussian
    eng.setTuning("mirror_share", 1)
    c = counters(eng)
    for k in (1, 10):
        assert_same(eng, queries, k, "k <= 10")
    d = delta(eng, c)
    assert d["mirror8_passes"] == 2 * len(queries) and d["mirror_passes"] == d["mirror8_passes"] and d["mirror_scans"] == d["mirror8_passes"]
    assert d["mirror8_fallbacks"] == 0 and d["mirror_scan_fallbacks"] == 0 and d["mirror8_unavailable"] == 0   # test_mirror8_cpu.py: every one certifies
    assert_same(eng, queries, 16, "k = 16")
    d = delta(eng, c)
    assert d["mirror8_passes"] == 3 * len(queries) and d["mirror8_fallbacks"] == 0 and d["mirror8_conversions"] == 0
    c = counters(eng)
    for k in (17, 32):                       # beyond what 64 candidates certify: bf16
        assert_same(eng, queries[:3], k, "k > 16")
    d = delta(eng, c)
    assert d["mirror8_passes"] == 0 and d["mirror_scans"] == 6 and d["mirror_passes"] == 6


def test_groups_of_two_to_four_with_mixed_k(gaussian):
    eng, queries, n, dims = gaussian
    ks = [10, 1, 16, 10]
    for g in (2, 3, 4):
        f32 = run_group(eng, queries[:g], ks[:g], 0, 0)
        alone = run_group(eng, queries[:g], ks[:g], 2, 0)
        c = counters(eng)
        shared = run_group(eng, queries[:g], ks[:g], 2, 2)
        d = delta(eng, c)
        assert all(same(a, b) for a, b in zip(shared, f32)) and all(same(a, b) for a, b in zip(shared, alone)), g
        assert (d["mirror8_passes"], d["mirror_passes"], d["mirror_shared_passes"], d["mirror_scans"], d["mirror8_fallbacks"]) == (1, 1, 1, g, 0), d
    # one member with k > 16: the whole set takes bf16, the answers do not change
    ks = [10, 32, 1]
    f32 = run_group(eng, queries[:3], ks, 0, 0)
    c = counters(eng)
    shared = run_group(eng, queries[:3], ks, 2, 2)
    d = delta(eng, c)
    assert all(same(a, b) for a, b in zip(shared, f32))
    assert (d["mirror8_passes"], d["mirror_passes"], d["mirror_scans"]) == (0, 1, 3)
    eng.setTuning("mirror_share", 1)


def test_mirror_bits_16_restores_the_bf16_counters_and_bad_values_are_refused(gaussian):
    eng, queries, n, dims = gaussian
    eng.setTuning("mirror_bits", 16)
    c = counters(eng)
    assert_same(eng, queries[:3], 10, "mirror_bits 16")
    d = delta(eng, c)
    assert (d["mirror8_passes"], d["mirror_scans"], d["mirror_passes"], d["mirror8_conversions"]) == (0, 3, 3, 0)
    for bad in (4, 1, -8, 32):
        with pytest.raises(Exception):
            eng.setTuning("mirror_bits", bad)
    assert eng.getTuning("mirror_bits") == 16
    eng.setTuning("mirror_bits", 0)            # auto: "scan_mirror" 2 on a small store stays bf16
    c = counters(eng)
    assert_same(eng, queries[:2], 10, "mirror_bits 0")
    assert delta(eng, c)["mirror8_passes"] == 0
    eng.setTuning("mirror_bits", 8)


def test_row_base_and_three_shards(wax):
    dims, k, n = 384, 10, 20005
    corpus = R.corpus_for(0, n, dims)
    queries = R.queries_for(dims)
    eng = make_engine(wax, 0, dims, corpus, ids=np.arange(n, dtype=np.uint64) * 3 + 11)
    eng.setRowBase(123457)
    warm(eng, queries[0])
    c = counters(eng)
    assert_same(eng, queries[:4], k, "row_base")
    d = delta(eng, c)
    assert (d["mirror8_passes"], d["mirror8_fallbacks"]) == (4, 0)
    many = wax.HIPVectorEngine(dimensions=dims, devices=[0] * 3)
    many.setTuning("shard_min_mb", 0)
    many.setTuning("mirror_bits", 8)
    many.addBatch(np.arange(n, dtype=np.uint64), corpus)
    one = make_engine(wax, 0, dims, corpus, bits=16)
    for _ in range(3):
        answer(many, queries[0], k, 2)
    before = many.getTuning("mirror8_passes")
    assert before == 3 and many.getTuning("mirror8_conversions") == 3       # every shard built its own, at its third query
    for q in queries[:4]:
        assert same(answer(many, q, k, 2), answer(one, q, k, 0))
    assert many.getTuning("mirror8_passes") - before == 3 * 4 and many.getTuning("mirror8_fallbacks") == 0


def test_duplicates_fall_back_and_stay_exact(wax):
    q = R.queries_for(384)[0]
    eng = make_engine(wax, 0, 384, R.duplicate_store(q))
    warm(eng, q)
    c = counters(eng)
    for k in (1, 10, 16):
        assert_same(eng, [q], k, "duplicates")
    d = delta(eng, c)
    assert d["mirror8_passes"] == 3 and d["mirror8_fallbacks"] == 3 and d["mirror_scan_fallbacks"] == 3


def test_tight_cluster_trips_the_breaker_and_stays_exact(wax):
    queries = R.queries_for(384)
    eng = make_engine(wax, 0, 384, R.clustered_store(queries[0]))
    for _ in range(2):
        answer(eng, queries[0], 10, 2)         # two on bf16; the third builds
    c = counters(eng)
    for i in range(32):
        assert_same(eng, [queries[i % len(queries)]], 10, "clustered")
    d = delta(eng, c)
    assert d["mirror8_breaker_trips"] == 1 and d["mirror8_passes"] == 8 and d["mirror8_fallbacks"] == 8, d   # eight uncertified in a row open it
    assert d["mirror_scans"] == 32             # the rest rode bf16


def test_outlier_row_zero_rows_and_non_finite_inputs(wax):
    dims = 384
    queries = R.queries_for(dims)
    eng = make_engine(wax, 0, dims, R.outlier_store())
    warm(eng, queries[0])
    c = counters(eng)
    for q in queries:
        assert_same(eng, [q], 10, "outlier element")
        assert R.OUTLIER_ROW in answer(eng, q, 10, 2)[0]
    d = delta(eng, c)
    assert d["mirror8_fallbacks"] == 0 and d["mirror8_passes"] == 2 * len(queries)
    eng = make_engine(wax, 0, dims, R.zero_row_store())
    warm(eng, queries[0])
    c = counters(eng)
    for k in (1, 10, 16):
        assert_same(eng, queries[:2], k, "zero rows")
    assert delta(eng, c)["mirror8_fallbacks"] == 0
    for metric in (0, 1):
        odd = R.corpus_for(metric, 5003, dims, seed=43).copy()
        odd[7, 3] = np.inf
        odd[9, 11] = np.nan
        odd[4000:4100] = 0.0
        eng = make_engine(wax, metric, dims, odd)
        warm(eng, queries[0])
        c = counters(eng)
        for k in (1, 10, 16):
            assert_same(eng, queries[:2], k, f"inf / NaN rows, metric {metric}")
        nq = queries[0].copy()
        nq[3] = np.nan
        f = delta(eng, c)["mirror8_fallbacks"]
        assert_same(eng, [nq], 10, f"NaN query, metric {metric}")
        d = delta(eng, c)
        assert d["mirror8_passes"] == 7 and d["mirror8_fallbacks"] == f + 1


def test_mutations_between_queries(wax):
    dims, k, n = 384, 10, 20005
    eng = make_engine(wax, 0, dims, R.corpus_for(0, n, dims))
    queries = R.queries_for(dims)
    warm(eng, queries[0])
    # append: only the appended rows are converted, at once
    c = counters(eng)
    eng.addBatch(np.array([900001, 900002], dtype=np.uint64), np.stack([queries[1], queries[2]]))
    assert_same(eng, queries[:3], k, "append")
    d = delta(eng, c)
    assert (d["mirror8_conversions"], d["mirror8_rows_converted"], d["mirror8_passes"]) == (1, 2, 3), d
    assert answer(eng, queries[1], k, 2)[0][0] == 900001
    count = n + 2

    def stale_then_rebuilt(ctx, count):
        c = counters(eng)
        assert_same(eng, queries[:2], k, ctx)           # the next two take bf16
        d = delta(eng, c)
        assert (d["mirror8_passes"], d["mirror8_conversions"], d["mirror_scans"]) == (0, 0, 2), (ctx, d)
        assert_same(eng, queries[2:5], k, ctx)          # the third rebuilds the whole code mirror
        d = delta(eng, c)
        assert (d["mirror8_passes"], d["mirror8_conversions"], d["mirror8_rows_converted"]) == (3, 1, count), (ctx, d)

    eng.addBatch(np.array([17], dtype=np.uint64), (queries[3] * 1.5)[None, :])      # upsert of a coded row
    stale_then_rebuilt("upsert", count)
    assert answer(eng, queries[3], k, 2)[0][0] == 17
    eng.remove(900001)
    count -= 1
    stale_then_rebuilt("remove", count)
    assert eng.removeBatch([5, 900002, 19999, 123]) == 4
    count -= 4
    stale_then_rebuilt("removeBatch", count)
    eng.reserve(eng.count * 4)                                                          # a new store slab
    eng.addBatch(np.arange(10**6, 10**6 + 500, dtype=np.uint64), R.corpus_for(0, 500, dims, seed=21))
    count += 500
    stale_then_rebuilt("growth", count)
    other = make_engine(wax, 0, dims, R.corpus_for(0, 8000, dims, seed=33))
    eng.deserialize(other.serialize())
    stale_then_rebuilt("deserialize", 8000)


@pytest.mark.timeout(600)
def test_ten_million_rows_auto_mode(wax):
    import torch
    import oracle
    n, dims, k = 10_000_000, 384, 10
    dev = torch.device("cuda", 0)
    eng = wax.HIPVectorEngine(dimensions=dims)
    eng.reserve(n)
    g = torch.Generator(device=dev)
    for lo in range(0, n, 1 << 20):
        g.manual_seed(oracle.CORPUS_SEED + lo)
        x = torch.randn((min(1 << 20, n - lo), dims), generator=g, device=dev, dtype=torch.float32)
        eng.addBatchDevice(np.arange(lo, lo + x.shape[0], dtype=np.uint64), torch.nn.functional.normalize(x, dim=1).contiguous())
    del x
    torch.cuda.synchronize()
    queries = R.queries_for(dims, 5)
    assert eng.getTuning("mirror_bits") == 0 and eng.getTuning("scan_mirror") == 1
    for q in queries[:2]:
        answer(eng, q, k, 1)                   # the two that find no code mirror (bf16)
    c = counters(eng)
    auto = [answer(eng, q, k, 1) for q in queries[2:]]
    d = delta(eng, c)
    assert (d["mirror8_passes"], d["mirror8_fallbacks"], d["mirror8_conversions"], d["mirror8_rows_converted"], d["mirror_scans"]) == (3, 0, 1, n, 3), d
    for q, a in zip(queries[2:], auto):
        assert same(a, answer(eng, q, k, 0))
