"""Single queries on the bf16 mirror ("scan_mirror"): the answer must be the f32 scan's, bit for bit, whether the certificate
held (the 64 best mirror rows re-scored in f32) or failed (the query re-run on the f32 scan at collect)."""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def wax(hip_lib):
    import wax_amd
    if hip_lib.wax_hip_device_count() == 0:
        pytest.skip("no HIP device on this host: the gpu-marked tests run on the MI355X box (pytest -m gpu)")
    assert hip_lib.wax_hip_available() == 1, "a HIP device is visible but it is not gfx950: the HIP path needs an MI355X"
    return wax_amd


def make_engine(wax, metric, dims, corpus=None, ids=None, **kw):
    eng = wax.HIPVectorEngine(metric=wax.VectorMetric(metric), dimensions=dims, **kw)
    if corpus is not None and len(corpus):
        eng.addBatch(np.arange(len(corpus), dtype=np.uint64) if ids is None else ids, corpus)
    return eng


def corpus_for(metric, n, dims, seed=0):
    x = oracle.gaussian_unit_rows(seed, n, dims)
    if metric == 1:   # dot: rows of different norms
        x = x * np.random.default_rng(seed + 7).uniform(0.5, 2.0, size=(n, 1)).astype(np.float32)
    return np.ascontiguousarray(x, dtype=np.float32)


def answer(eng, q, k, mode):
    eng.setTuning("scan_mirror", mode)
    return eng.searchArrays(q, k)


def assert_same(eng, queries, k, ctx):
    """Every query through the mirror (scan_mirror = 2) and through the f32 scan (0): the same ids and scores."""
    for i, q in enumerate(queries):
        m = answer(eng, q, k, 2)
        f = answer(eng, q, k, 0)
        assert np.array_equal(m[0], f[0]) and np.array_equal(m[1], f[1]), f"{ctx}: query {i}, k={k}"


def counters(eng):
    return {n: eng.getTuning(n) for n in ("mirror_scans", "mirror_scan_fallbacks", "mirror_scan_unavailable")}


@pytest.mark.parametrize("dims", [384, 768])
@pytest.mark.parametrize("metric", [0, 1], ids=["cosine", "dot"])
def test_mirror_answers_equal_the_f32_scan(wax, metric, dims):
    corpus = corpus_for(metric, 20000, dims)
    eng = make_engine(wax, metric, dims, corpus)
    queries = oracle.gaussian_unit_queries(4, dims)
    before = counters(eng)
    for k in (1, 10, 32):
        assert_same(eng, queries, k, f"metric {metric} dims {dims}")
    after = counters(eng)
    assert after["mirror_scans"] - before["mirror_scans"] == 3 * len(queries)
    assert after["mirror_scan_unavailable"] == before["mirror_scan_unavailable"]


def test_auto_mode_keeps_small_stores_and_other_shapes_on_the_f32_scan(wax):
    dims = 384
    eng = make_engine(wax, 0, dims, corpus_for(0, 5000, dims))
    q = oracle.gaussian_unit_queries(1, dims)[0]
    eng.setTuning("scan_mirror", 1)
    eng.searchArrays(q, 10)
    eng.setTuning("scan_mirror", 2)
    eng.searchArrays(q, 33)                 # k > 32
    eng.setTuning("force_general", 1)
    eng.searchArrays(q, 10)
    eng.setTuning("force_general", 0)
    assert eng.getTuning("mirror_scans") == 0
    l2 = make_engine(wax, 2, dims, corpus_for(0, 5000, dims))
    l2.setTuning("scan_mirror", 2)
    l2.searchArrays(q, 10)
    assert l2.getTuning("mirror_scans") == 0
    with pytest.raises(Exception):
        eng.setTuning("scan_mirror", 3)


def test_pipelined_submit_collect_and_row_base(wax):
    dims, k = 384, 10
    corpus = corpus_for(0, 30000, dims, seed=3)
    eng = make_engine(wax, 0, dims, corpus, ids=np.arange(30000, dtype=np.uint64) * 3 + 11)
    queries = oracle.gaussian_unit_queries(12, dims)
    want = [answer(eng, q, k, 0) for q in queries]
    eng.setTuning("scan_mirror", 2)
    got, pending = [], []
    for q in queries:
        if len(pending) == 4:
            got.append(eng.collect(pending.pop(0), k))
        pending.append(eng.submit(q, k))
    while pending:
        got.append(eng.collect(pending.pop(0), k))
    for g, w in zip(got, want):
        assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1])
    eng.setRowBase(123457)
    assert_same(eng, queries[:4], k, "row_base")


def test_three_shard_handle(wax):
    dims, k, n = 384, 10, 30000
    corpus = corpus_for(0, n, dims, seed=5)
    many = wax.HIPVectorEngine(dimensions=dims, devices=[0] * 3)
    many.setTuning("shard_min_mb", 0)
    many.addBatch(np.arange(n, dtype=np.uint64), corpus)
    one = make_engine(wax, 0, dims, corpus)
    queries = oracle.gaussian_unit_queries(4, dims)
    assert_same(many, queries, k, "3 shards")
    for q in queries:
        a = answer(many, q, k, 2)
        b = answer(one, q, k, 0)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert many.getTuning("mirror_scans") >= 3 * 2 * len(queries)


def test_mutations_between_queries(wax):
    dims, k = 384, 10
    rng = np.random.default_rng(11)
    corpus = corpus_for(0, 20000, dims, seed=9)
    eng = make_engine(wax, 0, dims, corpus)
    queries = oracle.gaussian_unit_queries(3, dims)
    assert_same(eng, queries, k, "initial")
    # add: a row equal to the first query becomes its best answer
    eng.addBatch(np.array([900001], dtype=np.uint64), queries[:1])
    assert_same(eng, queries, k, "add")
    assert answer(eng, queries[0], k, 2)[0][0] == 900001
    # upsert: rows that were mirrored are overwritten
    for r in rng.choice(20000, 50, replace=False):
        eng.addBatch(np.array([r], dtype=np.uint64), queries[1:2] * (1.0 + r / 1e5))
    assert_same(eng, queries, k, "upsert")
    # remove: the store's tail (and the mirror's) moves down
    for fid in (5, 900001, 17, 19999):
        eng.remove(int(fid))
    assert_same(eng, queries, k, "remove")
    # reserve growth: a new store slab, the mirror follows
    eng.reserve(eng.count * 4)
    eng.addBatch(np.arange(10**6, 10**6 + 500, dtype=np.uint64), corpus_for(0, 500, dims, seed=21))
    assert_same(eng, queries, k, "growth")
    # deserialize: every row is new
    blob = eng.serialize()
    other = make_engine(wax, 0, dims)
    other.deserialize(blob)
    assert_same(other, queries, k, "deserialize")
    eng.deserialize(make_engine(wax, 0, dims, corpus_for(0, 8000, dims, seed=33)).serialize())
    assert_same(eng, queries, k, "deserialize over a mirrored store")


def test_adversarial_stores_take_the_fallback_and_stay_exact(wax):
    dims = 384
    q = oracle.gaussian_unit_queries(1, dims)[0]
    base = corpus_for(0, 10000, dims, seed=41)
    before = 0
    # more than 64 exact duplicates of the answer row: 64 approximate candidates cannot certify the k-th
    dup = base.copy()
    dup[100:200] = q
    eng = make_engine(wax, 0, dims, dup)
    for k in (1, 10, 32):
        assert_same(eng, [q], k, "duplicates")
    assert eng.getTuning("mirror_scan_fallbacks") > before
    # zero rows and NaN rows; a NaN query
    odd = base.copy()
    odd[20:9990] = 0.0
    odd[9990:] = np.nan
    eng = make_engine(wax, 0, dims, odd)
    for k in (1, 10, 32):
        assert_same(eng, [q], k, "zero / NaN rows")
    nq = q.copy()
    nq[3] = np.nan
    assert_same(eng, [nq], 10, "NaN query")
    assert eng.getTuning("mirror_scan_fallbacks") > 0
    for metric in (0, 1):
        e2 = make_engine(wax, metric, dims, corpus_for(metric, 5000, dims, seed=43))
        assert_same(e2, [nq], 10, f"NaN query, metric {metric}")
        assert e2.getTuning("mirror_scan_fallbacks") >= 1
    # a clustered corpus: every row within a hair of one centre
    rng = np.random.default_rng(45)
    centre = q / np.linalg.norm(q)
    clustered = (centre[None, :] + 1e-3 * rng.standard_normal((10000, dims))).astype(np.float32)
    eng = make_engine(wax, 0, dims, clustered)
    for k in (1, 10, 32):
        assert_same(eng, [q], k, "clustered")
    assert eng.getTuning("mirror_scan_fallbacks") > 0


@pytest.mark.timeout(600)
def test_ten_million_rows_auto_mode(wax):
    import torch
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
    queries = oracle.gaussian_unit_queries(6, dims)
    auto = [answer(eng, q, k, 1) for q in queries]
    assert eng.getTuning("mirror_scans") == len(queries)
    assert eng.getTuning("mirror_scan_fallbacks") == 0
    for q, a in zip(queries, auto):
        f = answer(eng, q, k, 0)
        assert np.array_equal(a[0], f[0]) and np.array_equal(a[1], f[1])
    assert eng.getTuning("mirror_scans") == len(queries)
