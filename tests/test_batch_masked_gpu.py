"""searchBatchMasked ("The masked batch pass"): a batch under one row predicate from one bf16 MFMA pass over the mirror.
Held to a float64 model (mask the rows, the metric's distance, the k best by (distance, row)) under the project's 1e-5 / 2e-5 rule,
and bit for bit to searchBatchFiltered with the same arguments.

Rows and queries are iid Gaussian directions of unit norm, so similarities spread with sigma = 1 / sqrt(D) (0.051 at 384-d, 0.036 at
768-d) and eps is about 0.004 - 0.005. Every certified case keeps the bound of the rows a list dropped (the 17th best of a half-wave's
passing rows of one share) or the merge's cut (the 128th best listed row) at least 0.55 sigma below the exact k-th, several times
eps plus the spread of either order statistic: grid 1 goes with k = 1, k = 10 with grids of 2 or more, k = 32 with the default
grid, where a half-wave list sees at most 32 rows."""
import numpy as np
import pytest

from helpers import assert_parity

pytestmark = pytest.mark.gpu
COS, DOT, L2 = 0, 1, 2
USER = 0x100          # a flag no row carries: a predicate on it passes every row


@pytest.fixture(scope="module")
def wax(hip_lib):
    import wax_amd
    if hip_lib.wax_hip_device_count() == 0:
        pytest.skip("no HIP device on this host: the gpu-marked tests run on the MI355X box (pytest -m gpu)")
    return wax_amd


def unit_rows(n, dims, seed):
    v = np.random.default_rng(seed).standard_normal((n, dims))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def attributes(n, seed):
    """ts = row; bit 0 on a random half, bit 1 on every row but one, bit 2 on every row but five others."""
    rng = np.random.default_rng(seed)
    flags = (rng.random(n) < 0.5).astype(np.uint32) | 2 | 4
    odd = rng.choice(n, 6, replace=False)
    flags[odd[0]] &= ~np.uint32(2)
    flags[odd[1:]] &= ~np.uint32(4)
    return np.arange(n, dtype=np.int64), flags


def make_engine(wax, metric, dims, corpus, seed, **kw):
    eng = wax.HIPVectorEngine(metric=wax.VectorMetric(metric), dimensions=dims, **kw)
    ids = np.arange(len(corpus), dtype=np.uint64)
    eng.addBatch(ids, corpus)
    ts, flags = attributes(len(corpus), seed)
    eng.setAttributes(ids, ts, flags)
    return eng, corpus, ts, flags


STORES = {"a": (COS, 384, 9999), "b": (DOT, 768, 4097), "c": (DOT, 384, 257), "d": (COS, 768, 257)}


@pytest.fixture(scope="module")
def stores(wax):
    return {name: make_engine(wax, m, d, unit_rows(n, d, 7 + d + n), n) for name, (m, d, n) in STORES.items()}


def masks(n):
    lo = (n // 2) // 32 * 32   # whole 32-row tiles outside the window
    return {"all": (None, USER), "none": (None, 6), "one": (None, 2), "few": (None, 4), "half": (None, 1),
            "sixteenth": ((lo, lo + n // 16), 0), "window": ((n // 4, 3 * n // 4), 1)}


def check(store, metric, nq, k, grid, mask, min_score=None, queries=None):
    eng, corpus, ts, flags = store
    n, dims = corpus.shape
    time_range, deny = masks(n)[mask]
    queries = unit_rows(nq, dims, 1000 + nq + k) if queries is None else queries
    ids, scores, counts, st = eng.searchBatchMasked(queries, k, timeRange=time_range, denyFlags=deny, minScore=min_score, stats=True, grid=grid)
    f_ids, f_scores, f_counts = eng.searchBatchFiltered(queries, k, timeRange=time_range, denyFlags=deny, minScore=min_score)
    passing = (flags & deny) == 0
    if time_range is not None:
        passing &= (ts >= time_range[0]) & (ts < time_range[1])
    print(f"n {n} dims {dims} metric {metric} nq {nq} k {k} grid {grid} mask {mask}: {st}")
    assert st["route"] == 1 and st["passing_rows"] == passing.sum() and st["certified"] + st["rerun"] == nq
    assert np.array_equal(ids, f_ids) and np.array_equal(scores, f_scores) and np.array_equal(counts, f_counts)
    rows = np.flatnonzero(passing)
    sims = queries.astype(np.float64) @ corpus[rows].astype(np.float64).T
    if metric == DOT:
        sims -= 1.0                                                           # the score of distance 1 - q.v
    else:
        sims /= np.linalg.norm(queries.astype(np.float64), axis=1)[:, None] * np.linalg.norm(corpus[rows].astype(np.float64), axis=1)[None, :]
    cuts = np.full(nq, -np.inf) if min_score is None else np.array([-np.inf if m is None else m for m in np.broadcast_to(min_score, nq)])
    for q in range(nq):
        order = np.lexsort((rows, -sims[q]))[:k + 8]
        kept = [i for i in order[:k] if not np.float32(sims[q, i]) < np.float32(cuts[q])]
        assert_parity(ids[q, :counts[q]], scores[q, :counts[q]], rows[kept], sims[q, kept],
                      all_exp_scores=sims[q, order] if len(kept) == min(k, len(rows)) else None, ctx=f"query {q}")
        assert min_score is not None or (not ids[q, counts[q]:].any() and not scores[q, counts[q]:].any())   # (a cut leaves what it dropped behind the count, as the filtered batch does)
    return st


CASES = [("a", 256, 10, 0, "all"), ("a", 257, 10, 3, "half"), ("a", 33, 1, 1, "half"), ("a", 31, 10, 2, "window"),
         ("a", 1, 32, 0, "sixteenth"), ("a", 33, 10, 0, "none"), ("a", 31, 10, 1, "one"), ("a", 33, 10, 2, "few"),
         ("b", 33, 10, 3, "half"), ("b", 256, 32, 0, "all"), ("b", 31, 1, 1, "sixteenth"),
         ("c", 33, 10, 0, "half"), ("c", 1, 10, 2, "all"), ("d", 31, 1, 1, "half")]


@pytest.mark.parametrize("name,nq,k,grid,mask", CASES)
def test_masked_batch_equals_the_float64_model_and_the_filtered_batch(stores, name, nq, k, grid, mask):
    st = check(stores[name], STORES[name][0], nq, k, grid, mask)
    assert st["rerun"] == 0, st
    if mask == "sixteenth":
        assert st["tiles_skipped"] > 0
    if mask == "none":
        assert st["passing_rows"] == 0


def test_min_score_per_query_cuts_rows_and_counts(stores):
    cuts = [None if q % 3 == 0 else 0.13 + 0.01 * (q % 5) for q in range(33)]
    check(stores["a"], COS, 33, 10, 3, "half", min_score=cuts)
    check(stores["a"], COS, 33, 10, 3, "half", min_score=0.15)


def test_duplicates_of_the_best_row_are_refused_and_re_run(wax):
    """64 copies of the best row are 64 equal approximate and exact distances: one share lists 32 of them and the bound of the rest
    equals the k-th, which the strict certificate refuses."""
    corpus = unit_rows(257, 384, 3)
    corpus[:64] = corpus[200]
    eng, _, _, _ = store = make_engine(wax, COS, 384, corpus, 3)
    queries = np.repeat(corpus[200:201], 2, axis=0)
    st = check(store, COS, 2, 10, 1, "all", queries=queries)
    assert st["rerun"] > 0
    ids, _, _ = eng.searchBatchMasked(queries, 10, denyFlags=USER, grid=1)
    assert (ids == np.arange(10)).all()


def test_l2_large_k_and_a_sharded_handle_are_forwarded(wax, stores):
    l2 = make_engine(wax, L2, 384, unit_rows(257, 384, 5), 5)
    sharded = make_engine(wax, COS, 384, unit_rows(300, 384, 6), 6, devices=[0, 0, 0])
    for store, k in ((l2, 10), (stores["a"], 33), (sharded, 10)):
        queries = unit_rows(5, store[1].shape[1], 9)
        ids, scores, counts, st = store[0].searchBatchMasked(queries, k, denyFlags=1, stats=True)
        f_ids, f_scores, f_counts = store[0].searchBatchFiltered(queries, k, denyFlags=1)
        assert st["route"] == 0 and (counts > 0).all()
        assert np.array_equal(ids, f_ids) and np.array_equal(scores, f_scores) and np.array_equal(counts, f_counts)
