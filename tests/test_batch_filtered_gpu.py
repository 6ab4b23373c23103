"""Batched filtered search (wax_hip_search_batch_filtered / searchBatchFiltered): every row must equal what searchFiltered returns
for that query, its allow-list and its cut — ids, scores and counts bit for bit — whether the gather pass or the per-query path
answered it."""
import threading

import numpy as np
import pytest

import oracle
from helpers import assert_parity

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


def random_list(rng, n_rows, length):
    """`length` ids of which ~5 % are not in the engine (ids >= n_rows) and a few repeat."""
    if length == 0:
        return np.zeros(0, dtype=np.uint64)
    if length >= n_rows:
        ids = rng.permutation(n_rows).astype(np.uint64)
    else:
        ids = rng.choice(n_rows, size=length, replace=False).astype(np.uint64)
    m = max(1, length // 20) if length > 1 else 0
    if m:
        ids[:m] = rng.integers(n_rows, 2 * n_rows + 10 ** 6, size=m, dtype=np.uint64)       # absent ids
        ids[m:2 * m] = ids[len(ids) - m:] if len(ids) >= 3 * m else ids[m:2 * m]             # duplicates
    return rng.permutation(ids)


def loop(eng, queries, k, lists, cuts):
    out = []
    for q in range(len(queries)):
        lst = None if lists is None else lists[q]
        cut = None if cuts is None else cuts[q]
        out.append(eng.searchFiltered(queries[q], k, frameIds=lst, minScore=cut))
    return out


def assert_rows_equal(batch, ref, ctx):
    ids, scores, counts = batch
    for q, (ri, rs) in enumerate(ref):
        n = int(counts[q])
        assert n == len(ri), f"{ctx}: query {q} count {n} != {len(ri)}"
        assert np.array_equal(ids[q, :n], ri), f"{ctx}: query {q} ids"
        assert np.array_equal(scores[q, :n], rs), f"{ctx}: query {q} scores"


@pytest.fixture(scope="module")
def big(wax):
    n, dims = 1_000_000, 384
    corpus = corpus_for(0, n, dims)
    eng = make_engine(wax, 0, dims, corpus)
    yield eng, corpus
    eng.close()


def test_batch_equals_loop_on_1m_rows(wax, big):
    eng, corpus = big
    n = len(corpus)
    rng = np.random.default_rng(11)
    nq = 256
    queries = oracle.gaussian_unit_queries(nq, 384)
    lengths = [0, 1, 7, 100, 4095, 4096, 50000, n]
    lists = [random_list(rng, n, lengths[q % len(lengths)]) for q in range(nq)]
    for k in (1, 10, 100, 192):
        before = eng.getTuning("filter_batch_queries")
        got = eng.searchBatchFiltered(queries, k, frameIds=lists)
        assert eng.getTuning("filter_batch_queries") - before == nq
        assert_rows_equal(got, loop(eng, queries, k, lists, None), f"k={k}")


@pytest.mark.parametrize("metric,dims", [(1, 384), (2, 384), (0, 768)], ids=["dot384", "l2_384", "cos768"])
def test_metrics_and_dims_equal_loop(wax, metric, dims):
    n = 60000
    eng = make_engine(wax, metric, dims, corpus_for(metric, n, dims, seed=3))
    rng = np.random.default_rng(5)
    queries = oracle.gaussian_unit_queries(40, dims)
    lists = [random_list(rng, n, [10, 3000, 20000, 0][q % 4]) for q in range(40)]
    before = eng.getTuning("filter_batch_queries")
    assert_rows_equal(eng.searchBatchFiltered(queries, 10, frameIds=lists), loop(eng, queries, 10, lists, None), f"{metric}/{dims}")
    assert eng.getTuning("filter_batch_queries") - before == 40
    eng.close()


def test_unspecialised_dims_fall_back(wax):
    n, dims = 20000, 100
    eng = make_engine(wax, 0, dims, corpus_for(0, n, dims, seed=4))
    rng = np.random.default_rng(6)
    queries = oracle.gaussian_unit_queries(12, dims)
    lists = [random_list(rng, n, 500) for _ in range(12)]
    before = eng.getTuning("filter_batch_fallbacks")
    assert_rows_equal(eng.searchBatchFiltered(queries, 10, frameIds=lists), loop(eng, queries, 10, lists, None), "dims 100")
    assert eng.getTuning("filter_batch_fallbacks") - before == 12
    eng.close()


def test_mixed_batch_shared_lists_and_cuts(wax, big):
    eng, corpus = big
    n = len(corpus)
    rng = np.random.default_rng(21)
    shared = [random_list(rng, n, L) for L in (300, 5000, 20000, 80000)]
    nq = 256
    queries = oracle.gaussian_unit_queries(nq, 384)
    lists = [None if q >= 240 else shared[q % 4] for q in range(nq)]
    cuts = [[None, 0.05, float("nan"), float("inf"), -1.0][q % 5] for q in range(nq)]
    got = eng.searchBatchFiltered(queries, 10, frameIds=lists, minScore=cuts)
    assert_rows_equal(got, loop(eng, queries, 10, lists, cuts), "mixed")
    for q in range(nq):
        if cuts[q] == float("inf"):
            assert got[2][q] == 0
    # the 16 queries without a list and without a cut are their searchBatch rows
    plain = [q for q in range(240, nq) if cuts[q] is None or cuts[q] != cuts[q]]
    ids, scores, counts = eng.searchBatch(queries[plain], 10)
    for i, q in enumerate(plain):
        c = int(counts[i])
        assert int(got[2][q]) == c and np.array_equal(got[0][q, :c], ids[i, :c]) and np.array_equal(got[1][q, :c], scores[i, :c])


def test_large_k_takes_the_per_query_path(wax, big):
    eng, corpus = big
    rng = np.random.default_rng(31)
    queries = oracle.gaussian_unit_queries(6, 384)
    lists = [random_list(rng, len(corpus), L) for L in (200, 5000, 60000, 1000, 4096, 300000)]
    for k in (300, 1000):
        before = eng.getTuning("filter_batch_fallbacks")
        assert_rows_equal(eng.searchBatchFiltered(queries, k, frameIds=lists), loop(eng, queries, k, lists, None), f"k={k}")
        assert eng.getTuning("filter_batch_fallbacks") - before == 6


def test_ties_and_repeated_frame_ids(wax):
    dims = 128
    corpus = corpus_for(0, 5000, dims, seed=8)
    corpus[100:140] = corpus[99]                       # exact duplicates: ascending-row order
    eng = make_engine(wax, 0, dims, corpus)
    queries = np.ascontiguousarray(np.stack([corpus[99], corpus[7], corpus[1200]]), dtype=np.float32)
    lists = [np.arange(90, 200, dtype=np.uint64), np.arange(0, 5000, 3, dtype=np.uint64), None]
    assert_rows_equal(eng.searchBatchFiltered(queries, 50, frameIds=lists), loop(eng, queries, 50, lists, None), "duplicates")
    # a segment that holds one frame id in two rows: the lowest row answers, as in searchFiltered
    blob = bytearray(eng.serialize())
    n = eng.count
    tail = len(blob) - n * 8
    ids = np.frombuffer(bytes(blob[tail:]), dtype=np.uint64).copy()
    ids[2000:2010] = ids[1000:1010]
    blob[tail:] = ids.tobytes()
    eng2 = make_engine(wax, 0, dims)
    eng2.deserialize(bytes(blob))
    qs = np.ascontiguousarray(np.stack([corpus[2003], corpus[1005], corpus[10]]), dtype=np.float32)
    lists2 = [ids[995:1015].copy(), ids[1990:2020].copy(), np.arange(0, 3000, dtype=np.uint64)]
    assert_rows_equal(eng2.searchBatchFiltered(qs, 20, frameIds=lists2), loop(eng2, qs, 20, lists2, None), "repeated ids")
    eng.close()
    eng2.close()


def test_against_the_f64_oracle(wax):
    n, dims = 50000, 384
    corpus = corpus_for(0, n, dims, seed=12)
    eng = make_engine(wax, 0, dims, corpus)
    rng = np.random.default_rng(13)
    queries = oracle.gaussian_unit_queries(16, dims)
    lists = [random_list(rng, n, [50, 2000, 9000, 30000][q % 4]) for q in range(16)]
    ids, scores, counts = eng.searchBatchFiltered(queries, 10, frameIds=lists)
    frame_ids = np.arange(n, dtype=np.uint64)
    for q in range(16):
        rows = np.unique(lists[q][lists[q] < n]).astype(np.int64)
        ei, es, _, _ = oracle.search(0, corpus[rows], frame_ids[rows], queries[q], 10)
        _, es_all, _, _ = oracle.search(0, corpus[rows], frame_ids[rows], queries[q], 20)
        c = int(counts[q])
        assert c == len(ei)
        assert_parity(ids[q, :c], scores[q, :c], ei, es, all_exp_scores=es_all, ctx=f"query {q}")
    eng.close()


def test_sharded_handle_matches_single_engine(wax):
    n, dims = 30000, 384
    corpus = corpus_for(0, n, dims, seed=14)
    single = make_engine(wax, 0, dims, corpus)
    sharded = make_engine(wax, 0, dims, corpus, devices=[0, 0, 0])
    rng = np.random.default_rng(15)
    queries = oracle.gaussian_unit_queries(24, dims)
    lists = [None if q % 6 == 5 else random_list(rng, n, [20, 800, 7000, 25000, 0][q % 5]) for q in range(24)]
    cuts = [None if q % 3 else 0.1 for q in range(24)]
    a = single.searchBatchFiltered(queries, 10, frameIds=lists, minScore=cuts)
    b = sharded.searchBatchFiltered(queries, 10, frameIds=lists, minScore=cuts)
    assert_rows_equal(b, [(a[0][q, :a[2][q]], a[1][q, :a[2][q]]) for q in range(24)], "sharded")
    single.close()
    sharded.close()


def test_edges(wax):
    dims = 64
    corpus = corpus_for(0, 3000, dims, seed=16)
    eng = make_engine(wax, 0, dims, corpus)
    q = oracle.gaussian_unit_queries(4, dims)
    ids, scores, counts = eng.searchBatchFiltered(q[:0], 10, frameIds=[])
    assert ids.shape[0] == 0 and counts.shape == (0,)
    empty = make_engine(wax, 0, dims)
    _, _, c = empty.searchBatchFiltered(q, 10, frameIds=[[1, 2], None, [], [5]])
    assert (c == 0).all()
    empty.close()
    with pytest.raises(wax.EncodingError) as e1:
        eng.searchFiltered(q[0, :32], 10, frameIds=[1])
    with pytest.raises(wax.EncodingError) as e2:
        eng.searchBatchFiltered(q[:, :32], 10, frameIds=[[1]] * 4)
    assert str(e1.value) == str(e2.value)
    # out_stride < k keeps the best out_stride
    lists = [np.arange(0, 3000, 2, dtype=np.uint64)] * 4
    full = loop(eng, q, 40, lists, None)
    small = eng.searchBatchFiltered(q, 40, frameIds=lists)
    assert_rows_equal(small, full, "stride")
    import ctypes
    from wax_amd import _abi
    lib = _abi.lib()
    out_ids = np.zeros((4, 7), np.uint64)
    out_sc = np.zeros((4, 7), np.float32)
    cnt = np.zeros(4, np.uint32)
    flat = np.arange(0, 3000, 2, dtype=np.uint64)
    begin = np.zeros(4, np.uint64)
    length = np.full(4, flat.size, np.uint64)
    u64 = ctypes.POINTER(ctypes.c_uint64)
    f32 = ctypes.POINTER(ctypes.c_float)
    u32 = ctypes.POINTER(ctypes.c_uint32)
    qs = np.ascontiguousarray(q, np.float32)
    rc = lib.wax_hip_search_batch_filtered(eng._h, qs.ctypes.data_as(f32), 4, dims, 40, flat.ctypes.data_as(u64), flat.size,
                                           begin.ctypes.data_as(u64), length.ctypes.data_as(u64), None, out_ids.ctypes.data_as(u64),
                                           out_sc.ctypes.data_as(f32), 7, cnt.ctypes.data_as(u32))
    assert rc == _abi.OK
    for i in range(4):
        assert cnt[i] == 7 and np.array_equal(out_ids[i], full[i][0][:7]) and np.array_equal(out_sc[i], full[i][1][:7])
    length[2] = flat.size + 1   # leaves the id array
    rc = lib.wax_hip_search_batch_filtered(eng._h, qs.ctypes.data_as(f32), 4, dims, 40, flat.ctypes.data_as(u64), flat.size,
                                           begin.ctypes.data_as(u64), length.ctypes.data_as(u64), None, out_ids.ctypes.data_as(u64),
                                           out_sc.ctypes.data_as(f32), 7, cnt.ctypes.data_as(u32))
    assert rc == _abi.ERR_INVALID_ARGUMENT
    # two threads at once get the serial answers
    rng = np.random.default_rng(17)
    qq = oracle.gaussian_unit_queries(32, dims)
    tl = [random_list(rng, 3000, 400) for _ in range(32)]
    serial = eng.searchBatchFiltered(qq, 10, frameIds=tl)
    res = [None, None]

    def run(i):
        res[i] = [eng.searchBatchFiltered(qq, 10, frameIds=tl) for _ in range(5)]
    ts = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for r in res:
        for got in r:
            assert all(np.array_equal(a, b) for a, b in zip(got, serial))
    eng.close()
