"""searchBatchDims ("The K-split filtering GEMM"): cosine and dot batches at 1 024 and 1 536 dimensions with the one-pass
pipeline's filtering launch on batch_gemm_ks_kernel, held to searchBatch (the LDS-tiled route) bit for bit, to the float64 ranking,
and to a cap on the queries the exact ladder answers — a dropped or mis-paired K half would otherwise hide behind correct answers.
Run with -m gpu on an MI355X.

Every store has 65 613 rows: the smallest past the one-pass floor of 512 sampled 128-row tiles; its last 32-row tile holds 13 rows."""
import numpy as np
import pytest

from helpers import assert_parity

pytestmark = pytest.mark.gpu

COS, DOT, L2 = 0, 1, 2
N = 65613
ID0 = 7_000_000
TILE = 32


@pytest.fixture(scope="module")
def wax(hip_lib):
    import wax_amd
    if hip_lib.wax_hip_device_count() == 0:
        pytest.skip("no HIP device on this host: the gpu-marked tests run on the MI355X box (pytest -m gpu)")
    return wax_amd


def unit_rows(n, dims, seed):
    v = np.random.default_rng(seed).standard_normal((n, dims), dtype=np.float32)
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def make_engine(wax, corpus, metric, **kw):
    eng = wax.HIPVectorEngine(metric=wax.VectorMetric(metric), dimensions=corpus.shape[1], **kw)
    if kw:
        eng.setTuning("shard_min_mb", 0)
    eng.addBatch(np.arange(len(corpus), dtype=np.uint64) + ID0, corpus)
    return eng


@pytest.fixture(scope="module")
def store(wax):
    """(metric, dims) -> engine over Gaussian unit rows (scaled by linspace(0.6, 1.8) for dot) and the rows; built once."""
    cache = {}

    def get(metric, dims):
        if (metric, dims) not in cache:
            corpus = unit_rows(N, dims, 40 * dims + metric)
            if metric == DOT:
                corpus *= np.linspace(0.6, 1.8, N, dtype=np.float32)[:, None]
            eng = make_engine(wax, corpus, metric)
            eng.setRowBase(4096)
            cache[metric, dims] = eng, corpus
        return cache[metric, dims]
    return get


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("k", [1, 10, 32])
@pytest.mark.parametrize("dims", [1024, 1536])
@pytest.mark.parametrize("metric", [COS, DOT])
def test_equals_search_batch_and_the_float64_ranking(store, metric, dims, k):
    eng, corpus = store(metric, dims)
    nq = 301                                                     # pads to 512: four query groups
    queries = unit_rows(nq, dims, 977 + dims)
    before = eng.getTuning("batch_fallbacks")
    want = eng.searchBatch(queries, k)
    tiled_ladder = eng.getTuning("batch_fallbacks") - before
    *got, st = eng.searchBatchDims(queries, k, stats=True)
    print(metric, dims, k, st, "searchBatch's exact ladder:", tiled_ladder)
    assert st["route"] == 1 and st["queries"] == nq and st["tile_rows"] == TILE and st["queries_per_workgroup"] == 128, st
    assert st["workgroups"] == 256
    assert same(got, want)
    assert st["exact_ladder"] <= tiled_ladder + nq // 50, (st, tiled_ladder)
    ids, scores, counts = got
    v64 = corpus.astype(np.float64)
    for q in range(0, nq, nq // 6 + 1):
        sim = v64 @ queries[q].astype(np.float64)
        if metric == COS:
            sim /= np.linalg.norm(v64, axis=1) * np.linalg.norm(queries[q].astype(np.float64))
        order = np.lexsort((np.arange(N), -sim))[:k + 8]
        score = sim[order] if metric == COS else sim[order] - 1.0
        assert counts[q] == k
        assert_parity(ids[q], scores[q], ID0 + order[:k], score[:k], all_exp_scores=score, ctx=f"query {q}")


@pytest.mark.parametrize("dims", [1024, 1536])
def test_every_planted_position_is_found(store, dims):
    """Query i is a copy of store row P[i]: hit 0 is that row, hit 1 is searchBatch's. P: tile 0, the ragged last tile, the first and
    last row of each of the first 2 x per_group tiles (every bidx, and the second lap of the stride), the last 33 rows."""
    eng, corpus = store(COS, dims)
    per_group = 128                                              # nq <= 128 pads to 256: two query groups of 128 workgroups
    first = np.arange(2 * per_group) * TILE
    rows = np.unique(np.concatenate([np.arange(TILE), np.arange(N - N % TILE, N), first, first + TILE - 1, np.arange(N - 33, N)]))
    for at in range(0, len(rows), 128):
        part = rows[at:at + 128]
        for planted in (part, np.resize(part, 513)):             # 513 pads to 768: six query groups
            *got, st = eng.searchBatchDims(corpus[planted], 2, stats=True)
            assert st["route"] == 1 and st["workgroups"] == (256 if len(planted) <= 128 else 252), st
            assert np.array_equal(got[0][:, 0], ID0 + planted)
            assert same(got, eng.searchBatch(corpus[planted], 2))


@pytest.mark.parametrize("dims", [1024, 1536])
def test_rows_that_match_on_one_k_half(wax, dims):
    """Per query three planted rows: equal to the query on columns [0, D/2) and noise elsewhere, equal on [D/2, D), equal everywhere.
    They lead the answer in the float64 order, and no query needs the exact ladder: a wave half whose partial is lost or paired with
    another query's leaves the half rows at cosine ~ 0 in the filter."""
    corpus, queries = unit_rows(N, dims, 5 * dims), unit_rows(16, dims, 6 * dims)
    noise = unit_rows(32, dims, 7 * dims)
    at = np.random.default_rng(dims).choice(N, 48, replace=False).reshape(16, 3)
    h = dims // 2
    for q in range(16):
        corpus[at[q, 0]] = np.concatenate([queries[q, :h], noise[2 * q, h:]])
        corpus[at[q, 1]] = np.concatenate([noise[2 * q + 1, :h], queries[q, h:]])
        corpus[at[q, 2]] = queries[q]
    eng = make_engine(wax, corpus, COS)
    ids, scores, counts, st = eng.searchBatchDims(queries, 3, stats=True)
    print(dims, st)
    assert st["route"] == 1 and st["exact_ladder"] == 0, st
    for q in range(16):
        v64 = corpus[at[q]].astype(np.float64)
        cos = (v64 @ queries[q].astype(np.float64)) / (np.linalg.norm(v64, axis=1) * np.linalg.norm(queries[q].astype(np.float64)))
        order = np.argsort(-cos)
        assert order[0] == 2 and np.array_equal(ids[q], ID0 + at[q][order]), q
        assert np.max(np.abs(scores[q] - cos[order])) <= 1e-5, q


@pytest.mark.parametrize("metric,dims,n,shards", [(COS, 384, 5003, 0), (L2, 1024, 5003, 0), (COS, 1024, 5003, 0), (COS, 1024, 5003, 2)],
                         ids=["cos384", "l2-1024", "below-floor", "two-shards"])
def test_everything_else_is_forwarded(wax, metric, dims, n, shards):
    eng = make_engine(wax, unit_rows(n, dims, n + dims), metric, **({"devices": [0] * shards} if shards else {}))
    queries = unit_rows(40, dims, 3)
    *got, st = eng.searchBatchDims(queries, 10, stats=True)
    assert st["route"] == 0, st
    assert same(got, eng.searchBatch(queries, 10))
