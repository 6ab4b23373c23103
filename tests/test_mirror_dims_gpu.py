"""searchMirror ("The mirror pass at 512, 1 024 and 1 536 dimensions"): cosine and dot queries of 512-, 1 024- and 1 536-d
stores answered from shared passes over the bf16 mirror, certified in f32. Every answer is held bit for bit to the engine's own search
(searchArrays; searchFiltered under a predicate), its ids to the plain float64 ranking (1 - q.v / (|q| |v|) or 1 - q.v, ties by row)
and its scores to the float64 values within helpers.SCORE_TOL, the suite's bound for f32 against float64 on unit-scale data.

Rows and queries are Gaussian directions of unit norm, so the dot metric sees the margins the cosine metric does. With the seeds below
a float64 model of the pass (rows rounded to bf16, eps = max |v - bf16(v)| 1.001 + 3 D 2^-24 + 3e-6, about 0.0021) leaves
a_64 - eps - d_32 >= 0.0021 on every store and query here (1 536-d, 9 999 rows is the tightest; >= 0.012 at k = 10 under the two masks), three
orders of magnitude above the f32 roundings the model leaves out: every query must certify. The seeds also keep neighbouring float64
distances among the best 34 rows (the best 12 under a mask) at least 2.5e-6 apart (4e-6 at 512-d and 1 024-d), above what the f32
roundings of two distances can add up to (about 1e-6), so the f32 order is the float64 order."""
import numpy as np
import pytest

from helpers import SCORE_TOL

pytestmark = pytest.mark.gpu
COS, DOT, L2 = 0, 1, 2
ID0 = 1000                       # frame id of row 0
HALF, OUTSIDE, MOST = 0x100, 0x200, 0x400   # deny bits: a random half; the rows outside 1 000 .. 1 255; all rows but the first 40
SEED = {512: 12, 1024: 11, 1536: 88}


@pytest.fixture(scope="module")
def wax(hip_lib):
    import wax_amd
    if hip_lib.wax_hip_device_count() == 0:
        pytest.skip("no HIP device on this host: the gpu-marked tests run on the MI355X box (pytest -m gpu)")
    return wax_amd


def unit_rows(n, dims, seed):
    v = np.random.default_rng(seed).standard_normal((n, dims))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def make_engine(wax, corpus, metric, **kw):
    n = len(corpus)
    eng = wax.HIPVectorEngine(metric=wax.VectorMetric(metric), dimensions=corpus.shape[1], **kw)
    ids = np.arange(n, dtype=np.uint64) + ID0
    eng.addBatch(ids, corpus)
    flags = np.where(np.random.default_rng(n).random(n) < 0.5, HALF, 0).astype(np.uint32) | OUTSIDE | MOST
    flags[1000:1256] &= ~np.uint32(OUTSIDE)
    flags[:40] &= ~np.uint32(MOST)
    eng.setAttributes(ids, np.arange(n, dtype=np.int64), flags)
    return eng, flags


@pytest.fixture(scope="module")
def store(wax):
    """(dims, metric, rows) -> engine, flags, nine queries and their float64 distances to every row; built once."""
    cache = {}

    def get(dims, metric, n):
        if (dims, metric, n) not in cache:
            corpus, queries = unit_rows(n, dims, 1000 * SEED[dims] + dims + n), unit_rows(9, dims, 1000 * SEED[dims] + dims)
            v64, q64 = corpus.astype(np.float64), queries.astype(np.float64)
            sim = v64 @ q64.T
            if metric == COS:
                sim /= np.linalg.norm(v64, axis=1)[:, None] * np.linalg.norm(q64, axis=1)[None, :]
            cache[dims, metric, n] = make_engine(wax, corpus, metric) + (queries, np.ascontiguousarray((1.0 - sim).T))
        return cache[dims, metric, n]
    return get


def check(eng, metric, queries, d64, rows, k, deny, got):
    """row q of `got` against the engine's own search, bit for bit, and against the float64 ranking of `rows`"""
    ids, scores, counts = got
    for q in range(len(queries)):
        e_ids, e_scores = eng.searchFiltered(queries[q], k, denyFlags=deny) if deny else eng.searchArrays(queries[q], k)
        m = min(k, len(rows))
        assert counts[q] == m == len(e_ids)
        assert np.array_equal(ids[q, :m], e_ids) and np.array_equal(scores[q, :m], e_scores), q
        best = rows[np.lexsort((rows, d64[q][rows]))[:k]]
        assert np.array_equal(e_ids, ID0 + best), q
        want = 1.0 - d64[q][best] if metric == COS else -d64[q][best]
        assert np.max(np.abs(e_scores - want)) <= SCORE_TOL, q


@pytest.mark.parametrize("k", [1, 10, 32])
@pytest.mark.parametrize("n", [257, 4097, 9999])
@pytest.mark.parametrize("metric", [COS, DOT])
@pytest.mark.parametrize("dims", [512, 1024, 1536])
def test_equals_the_f32_scan_and_the_float64_reference(store, dims, metric, n, k):
    eng, _, queries, d64 = store(dims, metric, n)
    *got, st = eng.searchMirror(queries, k, returnStats=True)
    print(dims, metric, n, k, st)
    assert st["route"] == 1 and st["passes"] == 3 and st["lists"] >= 1
    check(eng, metric, queries, d64, np.arange(n), k, 0, got)
    assert st["certified"] == 9 and st["rerun"] == 0, st       # a pass that drops candidates cannot hide behind the re-run


@pytest.mark.parametrize("deny", [HALF, OUTSIDE])
@pytest.mark.parametrize("metric", [COS, DOT])
@pytest.mark.parametrize("dims", [512, 1024, 1536])
def test_masked_equals_the_predicate_search_and_the_float64_reference(store, dims, metric, deny):
    """OUTSIDE passes rows 1 000 .. 1 255: whole chunks are skipped, and the 16-row bitmap tile 992 .. 1 007 holds skipped and live
    chunks side by side (one 8-row chunk of each at 512-d)."""
    eng, flags, queries, d64 = store(dims, metric, 4097)
    *got, st = eng.searchMirror(queries[:5], 10, denyFlags=deny, returnStats=True)
    print(dims, metric, deny, st)
    assert st["route"] == 1 and st["passes"] == 2
    check(eng, metric, queries[:5], d64, np.flatnonzero((flags & deny) == 0), 10, deny, got)
    assert st["certified"] == 5, st
    assert deny != OUTSIDE or st["chunks_skipped"] > 0


@pytest.mark.parametrize("kind", ["identical", "few_passing"])
def test_what_cannot_certify_is_rerun(wax, store, kind):
    """identical: 300 copies of one row — the 64th key equals the k-th distance, ties go by ascending row. few_passing: 40 rows pass,
    fewer than the 64 candidates a certificate needs."""
    if kind == "identical":
        eng, _ = make_engine(wax, np.repeat(unit_rows(1, 512, 3), 300, axis=0), COS)
        queries, deny = unit_rows(4, 512, 4), 0
    else:
        (eng, _, queries, _), deny = store(512, COS, 4097), MOST
    ids, scores, counts, st = eng.searchMirror(queries[:4], 10, denyFlags=deny, returnStats=True)
    assert st["route"] == 1 and st["rerun"] == 4 and st["certified"] == 0, st
    for q in range(4):
        e_ids, e_scores = eng.searchFiltered(queries[q], 10, denyFlags=deny) if deny else eng.searchArrays(queries[q], 10)
        assert counts[q] == 10 and np.array_equal(ids[q], e_ids) and np.array_equal(scores[q], e_scores), q
        assert kind != "identical" or np.array_equal(ids[q], ID0 + np.arange(10))


@pytest.mark.parametrize("case", ["dims384", "l2", "k33", "sharded"])
def test_forwarded_shapes_return_the_existing_search(wax, case):
    dims, k = (384, 10) if case == "dims384" else (1024, 33 if case == "k33" else 10)
    eng, _ = make_engine(wax, unit_rows(300, dims, 31), L2 if case == "l2" else COS, **({"devices": [0, 0]} if case == "sharded" else {}))
    queries = unit_rows(5, dims, 32)
    for deny in (0, HALF):
        ids, scores, counts, st = eng.searchMirror(queries, k, denyFlags=deny, returnStats=True)
        assert st["route"] == 0 and st["passes"] == 0
        for q in range(5):
            e_ids, e_scores = eng.searchFiltered(queries[q], k, denyFlags=deny) if deny else eng.searchArrays(queries[q], k)
            assert counts[q] == len(e_ids) == k and np.array_equal(ids[q, :k], e_ids) and np.array_equal(scores[q, :k], e_scores)


def test_follows_an_append_a_removal_and_an_overwrite(wax):
    eng, _ = make_engine(wax, unit_rows(300, 1024, 21), COS)
    queries = unit_rows(5, 1024, 22)
    steps = [lambda: None,
             lambda: eng.addBatch(np.arange(100, dtype=np.uint64) + ID0 + 5000, unit_rows(100, 1024, 23)),
             lambda: eng.remove(ID0 + 17),
             lambda: eng.addBatch(np.array([ID0 + 200], dtype=np.uint64), queries[3:4])]     # a stored id: overwritten in place, now query 3's best row
    for step in steps:
        step()
        ids, scores, counts, st = eng.searchMirror(queries, 10, returnStats=True)
        assert st["route"] == 1 and st["passes"] == 2
        for q in range(5):
            e_ids, e_scores = eng.searchArrays(queries[q], 10)
            assert counts[q] == 10 and np.array_equal(ids[q], e_ids) and np.array_equal(scores[q], e_scores), (eng.count, q)
    assert ids[3, 0] == ID0 + 200
