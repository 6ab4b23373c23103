"""searchBatchL2 ("The register-resident L2 filter"): L2 batches at 384 and 768 dimensions with the one-pass pipeline's
filtering launch on batch_gemm_rq_l2_kernel, held to searchBatch (the LDS-tiled route) bit for bit, to the float64 ranking, and to a
cap on the queries the exact ladder answers — a norm slice paired with the wrong rows would otherwise hide behind correct answers.
Run with -m gpu on an MI355X.

Every store has 65 613 rows: the smallest past the planner's counted-list floor of 512 tiles of 128 rows; its last tile holds 13 rows
at both tile heights (64 rows at 384-d, 32 at 768-d). Rows and queries have norms spread over [0.5, 1.0]: the norm term decides rankings."""
import numpy as np
import pytest

from helpers import assert_parity

pytestmark = pytest.mark.gpu

COS, L2 = 0, 2
N = 65613
ID0 = 7_000_000
TILE = {384: 64, 768: 32}


@pytest.fixture(scope="module")
def wax(hip_lib):
    import wax_amd
    if hip_lib.wax_hip_device_count() == 0:
        pytest.skip("no HIP device on this host: the gpu-marked tests run on the MI355X box (pytest -m gpu)")
    return wax_amd


def shell_rows(n, dims, seed):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, dims))
    return (v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(0.5, 1.0, (n, 1))).astype(np.float32)


def make_engine(wax, corpus, metric=L2, **kw):
    eng = wax.HIPVectorEngine(metric=wax.VectorMetric(metric), dimensions=corpus.shape[1], **kw)
    if kw:
        eng.setTuning("shard_min_mb", 0)
    eng.addBatch(np.arange(len(corpus), dtype=np.uint64) + ID0, corpus)
    return eng


@pytest.fixture(scope="module")
def store(wax):
    """dims -> L2 engine over shell rows (row base 4 096) and the rows; built once."""
    cache = {}

    def get(dims):
        if dims not in cache:
            corpus = shell_rows(N, dims, 41 * dims)
            eng = make_engine(wax, corpus)
            eng.setRowBase(4096)
            cache[dims] = eng, corpus
        return cache[dims]
    return get


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("k", [1, 10, 32])
@pytest.mark.parametrize("dims", [384, 768])
def test_equals_search_batch_and_the_float64_ranking(store, dims, k):
    eng, corpus = store(dims)
    nq = 301                                                     # pads to 512: two query groups of 128 workgroups
    queries = shell_rows(nq, dims, 977 + dims)
    before = eng.getTuning("batch_fallbacks")
    want = eng.searchBatch(queries, k)
    tiled_ladder = eng.getTuning("batch_fallbacks") - before
    *got, st = eng.searchBatchL2(queries, k, stats=True)
    print(dims, k, st, "searchBatch's exact ladder:", tiled_ladder)
    assert st["route"] == 1 and st["queries"] == nq and st["tile_rows"] == TILE[dims] and st["queries_per_workgroup"] == 256, st
    assert st["workgroups"] == 256
    assert same(got, want)
    assert st["exact_ladder"] <= tiled_ladder + nq // 50, (st, tiled_ladder)
    ids, scores, counts = got
    v64 = corpus.astype(np.float64)
    for q in range(0, nq, nq // 6 + 1):
        d = ((v64 - queries[q].astype(np.float64)) ** 2).sum(1)
        order = np.lexsort((np.arange(N), d))[:k + 8]
        assert counts[q] == k
        assert_parity(ids[q], scores[q], ID0 + order[:k], -d[order[:k]], all_exp_scores=-d[order], ctx=f"query {q}")


@pytest.mark.parametrize("dims", [384, 768])
def test_every_planted_position_is_found(store, dims):
    """Query i is a copy of store row P[i]: hit 0 is that row, hit 1 is searchBatch's. P: tile 0, the ragged last tile, the first and
    last row of each of the first 2 x per_group tiles (every bidx, and the second lap of the stride), the last 33 rows."""
    eng, corpus = store(dims)
    tile, per_group = TILE[dims], 256                            # nq <= 128 pads to 256: one query group of 256 workgroups
    first = np.arange(2 * per_group) * tile
    rows = np.unique(np.concatenate([np.arange(tile), np.arange(N - N % tile, N), first, first + tile - 1, np.arange(N - 33, N)]))
    for at in range(0, len(rows), 128):
        part = rows[at:at + 128]
        for planted in (part, np.resize(part, 513)):             # 513 pads to 768: three query groups of 85 workgroups
            *got, st = eng.searchBatchL2(corpus[planted], 2, stats=True)
            assert st["route"] == 1 and st["workgroups"] == (256 if len(planted) <= 128 else 255) and st["exact_ladder"] == 0, st
            assert np.array_equal(got[0][:, 0], ID0 + planted)
            assert same(got, eng.searchBatch(corpus[planted], 2))


@pytest.mark.parametrize("dims", [384, 768])
def test_rows_are_paired_with_their_own_norm(wax, dims):
    """Per query: row r is a copy of the query, row r + 1 is 3 x the query (best by dot, far by L2), row r - 1 is 0.05 x noise. Hit 0 is
    row r and no query needs the exact ladder: a norm slice shifted by a row in either direction, or dropped, loses row r in the filter
    or puts row r + 1 among the candidates with a key the certificate cannot stand behind."""
    corpus, queries = shell_rows(N, dims, 5 * dims), shell_rows(16, dims, 6 * dims)
    at = np.random.default_rng(dims).choice((N - 3) // 3, 16, replace=False) * 3 + 1
    corpus[at], corpus[at + 1], corpus[at - 1] = queries, 3 * queries, 0.05 * shell_rows(16, dims, 7 * dims)
    eng = make_engine(wax, corpus)
    *got, st = eng.searchBatchL2(queries, 2, stats=True)
    print(dims, st)
    assert st["route"] == 1 and st["exact_ladder"] == 0, st
    assert np.array_equal(got[0][:, 0], ID0 + at)
    assert same(got, eng.searchBatch(queries, 2))


@pytest.mark.parametrize("metric,dims,n,shards", [(COS, 384, N, 0), (L2, 1024, N, 0), (L2, 384, 5003, 0), (L2, 384, N, 2)],
                         ids=["cos384", "l2-1024", "below-floor", "two-shards"])
def test_everything_else_is_forwarded(wax, metric, dims, n, shards):
    eng = make_engine(wax, shell_rows(n, dims, n + dims), metric, **({"devices": [0] * shards} if shards else {}))
    queries = shell_rows(40, dims, 3)
    *got, st = eng.searchBatchL2(queries, 10, stats=True)
    assert st["route"] == 0, st
    assert same(got, eng.searchBatch(queries, 10))
