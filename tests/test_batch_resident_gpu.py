"""searchBatchResident ("The resident batch"): one launch scores every (row, query) pair of a small store exactly.
Held to float64 within the f32 error of a D-term dot product, and bit for bit to search / searchBatch.

Inputs: rows and queries of norm in [0.5, 1], so every f32 distance is within BETA = 2 * D * 2^-24 of its float64 value (the
first-order bound of a D-term f32 dot product plus the finish) and a returned row lies within 2 * BETA of the true k-th distance."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
COS, DOT, L2 = 0, 1, 2


@pytest.fixture(scope="module")
def wax(hip_lib):
    import wax_amd
    if hip_lib.wax_hip_device_count() == 0:
        pytest.skip("no HIP device on this host: the gpu-marked tests run on the MI355X box (pytest -m gpu)")
    return wax_amd


def vectors(n, dims, seed):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, dims))
    return (v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(0.5, 1.0, (n, 1))).astype(np.float32)


def f64_distances(corpus, queries, metric):
    c, q = corpus.astype(np.float64), queries.astype(np.float64)
    dots = q @ c.T
    if metric == DOT:
        return 1.0 - dots
    if metric == L2:
        return (q * q).sum(1)[:, None] - 2.0 * dots + (c * c).sum(1)[None, :]
    norms = np.linalg.norm(q, axis=1)[:, None] * np.linalg.norm(c, axis=1)[None, :]
    live = (np.linalg.norm(q, axis=1)[:, None] > 1e-6) & (np.linalg.norm(c, axis=1)[None, :] > 1e-6)
    return 1.0 - np.where(live, dots / np.where(live, norms, 1.0), 0.0)


def make_engine(wax, metric, dims, corpus, **kw):
    eng = wax.HIPVectorEngine(metric=wax.VectorMetric(metric), dimensions=dims, **kw)
    eng.addBatch(np.arange(len(corpus), dtype=np.uint64), corpus)
    return eng


def check(eng, corpus, queries, k, metric, route=1):
    """The three claims for one call (frame id = row): float64, search per query (8 of them), searchBatch for the whole batch."""
    n, dims = corpus.shape
    ids, scores, counts, st = eng.searchBatchResident(queries, k, stats=True)
    assert st["route"] == route, st
    want = min(k, n)
    beta = 2.0 * dims * 2.0 ** -24
    d64 = f64_distances(corpus, queries, metric)
    kth = np.partition(d64, want - 1, axis=1)[:, want - 1]
    rows = ids[:, :want].astype(np.int64)
    got64 = np.take_along_axis(d64, rows, axis=1)
    dist = (1.0 - scores[:, :want].astype(np.float64)) if metric == COS else -scores[:, :want].astype(np.float64)
    print(f"n {n} nq {len(queries)} k {k} dims {dims} metric {metric}: {st}; worst score error {np.abs(dist - got64).max():.3g}, "
          f"worst excess over the k-th {(got64 - kth[:, None]).max():.3g}, beta {beta:.3g}")
    assert (counts == want).all()
    assert (got64 <= kth[:, None] + 2.0 * beta).all() and (np.abs(dist - got64) <= beta).all()
    assert all(len(set(r)) == want for r in rows.tolist())
    b_ids, b_scores, b_counts = eng.searchBatch(queries, k)
    assert np.array_equal(ids, b_ids) and np.array_equal(scores, b_scores) and np.array_equal(counts, b_counts)
    for qi in np.linspace(0, len(queries) - 1, min(8, len(queries))).astype(int):
        s_ids, s_scores = eng.searchArrays(queries[qi], k)
        assert np.array_equal(ids[qi, :counts[qi]], s_ids) and np.array_equal(scores[qi, :counts[qi]], s_scores), qi
    return st


@pytest.fixture(scope="module")
def base(wax):
    corpus = vectors(2600, 384, 1)
    return make_engine(wax, COS, 384, corpus), corpus


@pytest.mark.parametrize("nq", (1, 15, 16, 17, 256, 1025))
def test_query_counts(base, nq):
    st = check(base[0], base[1], vectors(nq, 384, 100 + nq), 10, COS)
    assert st["launches"] == (nq + 1023) // 1024 and st["query_blocks"] == (min(nq, 1024) + 15) // 16


@pytest.mark.parametrize("k", (1, 10, 64, 65, 192))
def test_top_k(base, k):
    check(base[0], base[1], vectors(17, 384, 7), k, COS)


@pytest.mark.parametrize("dims", (64, 128, 384, 768))
@pytest.mark.parametrize("metric", (COS, DOT, L2))
def test_dimensions_and_metrics(wax, dims, metric):
    corpus = vectors(2600, dims, dims + metric)
    check(make_engine(wax, metric, dims, corpus), corpus, vectors(17, dims, 3), 10, metric)


@pytest.mark.parametrize("dims", (64, 384, 768))
@pytest.mark.parametrize("which", ("one", "row-group", "shares-1", "T-1", "T", "T+1", "tile-per-share+1"))
def test_row_counts_at_the_edges_of_the_split(wax, dims, which):
    """n read from the split itself: T and the shares (of k = 64, so that a tile per share stays under the resident limit) from stats; n < k pads the output."""
    queries = vectors(17, dims, 5)
    st = make_engine(wax, COS, dims, vectors(64, dims, 0)).searchBatchResident(queries, 64, stats=True)[3]
    t, shares, group = st["tile_rows"], st["row_shares"], {64: 16, 384: 32, 768: 64}[dims]
    n = {"one": 1, "row-group": 64 // group, "shares-1": shares - 1, "T-1": t - 1, "T": t, "T+1": t + 1, "tile-per-share+1": shares * t + 1}[which]
    corpus = vectors(n, dims, n)
    assert n < 64 or check(make_engine(wax, COS, dims, corpus), corpus, queries, 64, COS)["row_shares"] == shares
    assert n >= 64 or check(make_engine(wax, COS, dims, corpus), corpus, queries, 64, COS)["route"] == 1


def test_forwarded_calls_answer_as_search_batch(wax, base):
    corpus = vectors(300, 100, 2)
    check(make_engine(wax, COS, 100, corpus), corpus, vectors(17, 100, 3), 10, COS, route=0)       # a dimension outside the table
    check(base[0], base[1], vectors(17, 384, 4), 500, COS, route=0)                                 # top_k > 192
    many = wax.HIPVectorEngine(metric=wax.VectorMetric(COS), dimensions=384, devices=[0] * 3)       # a handle over three shards
    many.addBatch(np.arange(len(base[1]), dtype=np.uint64), base[1])
    q = vectors(17, 384, 6)
    got, want = many.searchBatchResident(q, 10, stats=True), many.searchBatch(q, 10)
    assert got[3]["route"] == 0 and all(np.array_equal(a, b) for a, b in zip(got[:3], want))


def same_as_both(eng, queries, k):
    got = eng.searchBatchResident(queries, k, stats=True)
    assert got[3]["route"] == 1
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got[:3], eng.searchBatch(queries, k)))
    for qi, q in enumerate(queries):
        s_ids, s_scores = eng.searchArrays(q, k)
        assert np.array_equal(got[0][qi, :got[2][qi]], s_ids) and np.array_equal(got[1][qi, :got[2][qi]], s_scores, equal_nan=True), qi
    return got


@pytest.mark.parametrize("metric", (COS, L2))
def test_equal_rows_come_back_in_row_order(wax, metric):
    corpus = np.repeat(vectors(1, 384, 9), 300, axis=0)
    ids = same_as_both(make_engine(wax, metric, 384, corpus), vectors(17, 384, 10), 10)[0]
    assert (ids == np.arange(10, dtype=np.uint64)[None, :]).all()


def test_zero_row_zero_query_and_a_nan_query(wax):
    corpus, queries = vectors(700, 384, 11), vectors(17, 384, 12)
    corpus[5] = 0.0
    queries[3] = 0.0
    eng = make_engine(wax, COS, 384, corpus)
    clean = same_as_both(eng, queries, 10)
    queries[9, 100] = np.nan
    dirty = same_as_both(eng, queries, 10)
    others = np.arange(17) != 9
    assert all(np.array_equal(a[others], b[others]) for a, b in zip(clean[:3], dirty[:3]))


def test_keys_carry_the_global_row(wax):
    corpus, queries = vectors(700, 384, 13), vectors(17, 384, 14)
    eng = make_engine(wax, COS, 384, corpus)
    eng.setRowBase(1 << 20)
    want, want_counts = eng.searchBatchHits(queries, 10)
    hits, counts = np.empty_like(want), np.zeros(17, dtype=np.uint32)
    rc = eng._lib.wax_hip_search_batch_resident(eng._h, queries.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 17, 384, 10,
                                                hits.ctypes.data_as(ctypes.POINTER(wax._abi.Hit)), 10,
                                                counts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), None)
    assert rc == 0 and np.array_equal(hits, want) and np.array_equal(counts, want_counts)
    assert ((hits[:, :, 0] & 0xFFFFFFFF) >= (1 << 20)).all() and (hits[:, :, 1] < 700).all()


def test_after_mutations_it_answers_as_a_rebuilt_store(wax):
    corpus, queries = vectors(2600, 384, 15), vectors(17, 384, 16)
    eng = make_engine(wax, COS, 384, corpus)
    assert eng.removeBatch(np.arange(0, 2600, 3, dtype=np.uint64)) == 867
    fresh_row, upsert = vectors(2, 384, 17)
    eng.add(5000, fresh_row)
    eng.add(1, upsert)
    keep = np.array([i for i in range(2600) if i % 3], dtype=np.uint64)
    rows = corpus[keep.astype(np.int64)].copy()
    rows[0] = upsert                                            # frame 1 is the first surviving row
    rebuilt = wax.HIPVectorEngine(metric=wax.VectorMetric(COS), dimensions=384)
    rebuilt.addBatch(np.append(keep, np.uint64(5000)), np.vstack([rows, fresh_row[None, :]]))
    got, want = same_as_both(eng, queries, 10), rebuilt.searchBatchResident(queries, 10)
    assert all(np.array_equal(a, b) for a, b in zip(got[:3], want))
