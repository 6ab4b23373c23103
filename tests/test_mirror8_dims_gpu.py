"""searchMirror(bits=8) ("The code mirror at 512, 1 024 and 1 536 dimensions"): cosine and dot queries of 512-, 1 024- and
1 536-d stores answered from shared int8-MFMA passes over the 8-bit code mirror, certified in f32. Every answer is held bit for bit to
the engine's own search (searchArrays; searchFiltered under a predicate), its ids to the plain float64 ranking and its scores to the
float64 values within helpers.SCORE_TOL. Every case asserts route 1 with every query certified and none re-run: the re-run would hide
a pass that loses or mis-scores rows.

The candidate count comes from tests/mirror8_dims_model.py, a float64 model of the certificate dist(B) - Mirror8Slack > d_k on these
very inputs (unit Gaussian rows, the seeds below, nine queries, k = 16, cosine; `python tests/mirror8_dims_model.py` prints it).
Smallest margin over the nine queries, by candidates per query:
    dims  rows  slack      64       128      256      512      1024
     512   257  1.82e-4  0.0253   0.0552   0.1264   0.1264   0.1264
     512  4097  1.82e-4  0.0117   0.0251   0.0403   0.0571   0.0779
     512  9999  1.82e-4  0.0101   0.0211   0.0347   0.0484   0.0648
    1024   257  3.10e-4  0.0164   0.0370   0.0916   0.0916   0.0916
    1024  4097  3.10e-4  0.0066   0.0153   0.0240   0.0357   0.0503
    1024  9999  3.10e-4  0.0030   0.0097   0.0180   0.0287   0.0406
    1536   257  4.29e-4  0.0118   0.0271   0.0678   0.0678   0.0678
    1536  4097  4.29e-4  0.0020   0.0081   0.0166   0.0254   0.0370
    1536  9999  4.29e-4  0.0002   0.0063   0.0136   0.0213   0.0310
The per-row err stays near 0.008 while the spread of similarities shrinks as 1 / sqrt(D): 64 candidates leave half a slack at
1 536-d x 9 999 rows (and by the normal order statistics nothing at 10M rows), below ten slacks (0.0043) from 4 097 rows on and at
1 024-d x 9 999. 128 is the smallest count that clears ten slacks on every input here (0.0063 at the tightest, fourteen slacks), and
the count the finish runs at (MIRROR8_DIMS_C; mirror_wide.hip's selection, generic in its count): every query here must certify.
Under the masks at k = 10 the model leaves at least 0.0155 (HALF) and 0.0345 (OUTSIDE, 256 passing rows) at 128. MOST passes 40
rows: no list is full, B is the pad, every passing row is re-scored and the case checks only that the pass loses no row. Everywhere
else fewer rows are re-scored than may be offered (257 rows: 128 of them), so a mis-scored row can fall out of the candidates: those
cases and test_every_k_step_and_tile_position_counts hold the keys themselves."""
import numpy as np
import pytest

from helpers import SCORE_TOL

pytestmark = pytest.mark.gpu
COS, DOT, L2 = 0, 1, 2
ID0 = 1000                       # frame id of row 0
HALF, OUTSIDE, MOST = 0x100, 0x200, 0x400   # deny bits: a random half; the rows outside 1 000 .. 1 255; all rows but the first 40
SEED = {512: 12, 1024: 11, 1536: 88}
STATS8 = {"route", "passes", "certified", "rerun", "lists", "tiles_skipped", "candidates"}


@pytest.fixture(scope="module")
def wax(hip_lib):
    import wax_amd
    if hip_lib.wax_hip_device_count() == 0:
        pytest.skip("no HIP device on this host: the gpu-marked tests run on the MI355X box (pytest -m gpu)")
    return wax_amd


def unit_rows(n, dims, seed):
    v = np.random.default_rng(seed).standard_normal((n, dims))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def make_engine(wax, corpus, metric):
    n = len(corpus)
    eng = wax.HIPVectorEngine(metric=wax.VectorMetric(metric), dimensions=corpus.shape[1])
    ids = np.arange(n, dtype=np.uint64) + ID0
    eng.addBatch(ids, corpus)
    flags = np.where(np.random.default_rng(n).random(n) < 0.5, HALF, 0).astype(np.uint32) | OUTSIDE | MOST
    flags[1000:1256] &= ~np.uint32(OUTSIDE)
    flags[:40] &= ~np.uint32(MOST)
    eng.setAttributes(ids, np.arange(n, dtype=np.int64), flags)
    return eng, flags


def distances64(corpus, queries, metric):
    v64, q64 = corpus.astype(np.float64), queries.astype(np.float64)
    sim = v64 @ q64.T
    if metric == COS:
        sim /= np.linalg.norm(v64, axis=1)[:, None] * np.linalg.norm(q64, axis=1)[None, :]
    return np.ascontiguousarray((1.0 - sim).T)


@pytest.fixture(scope="module")
def store(wax):
    """(dims, metric, rows) -> engine, flags, nine queries and their float64 distances to every row; built once."""
    cache = {}

    def get(dims, metric, n):
        if (dims, metric, n) not in cache:
            corpus, queries = unit_rows(n, dims, 1000 * SEED[dims] + dims + n), unit_rows(9, dims, 1000 * SEED[dims] + dims)
            cache[dims, metric, n] = make_engine(wax, corpus, metric) + (queries, distances64(corpus, queries, metric))
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


@pytest.mark.parametrize("k", [1, 10, 16])
@pytest.mark.parametrize("n", [257, 4097, 9999])
@pytest.mark.parametrize("metric", [COS, DOT])
@pytest.mark.parametrize("dims", [512, 1024, 1536])
def test_equals_the_f32_scan_and_the_float64_reference(store, dims, metric, n, k):
    """nine queries: passes of 4, 4 and 1; a lone partial tile, more tiles than waves, a tail tile"""
    eng, _, queries, d64 = store(dims, metric, n)
    *got, st = eng.searchMirror(queries, k, returnStats=True, bits=8)
    print(dims, metric, n, k, st)
    assert set(st) == STATS8 and st["route"] == 1 and st["passes"] == 3 and st["lists"] >= 1 and st["candidates"] == 128
    check(eng, metric, queries, d64, np.arange(n), k, 0, got)
    assert st["certified"] == 9 and st["rerun"] == 0, st


@pytest.mark.parametrize("deny", [HALF, OUTSIDE, MOST])
@pytest.mark.parametrize("metric", [COS, DOT])
@pytest.mark.parametrize("dims,n", [(512, 9999), (1024, 4097), (1536, 4097)])
def test_masked_equals_the_predicate_search_and_the_float64_reference(store, dims, n, metric, deny):
    """OUTSIDE passes rows 1 000 .. 1 255: every tile but seventeen is skipped, and tiles 62 and 78 hold passing and denied rows"""
    eng, flags, queries, d64 = store(dims, metric, n)
    *got, st = eng.searchMirror(queries[:5], 10, denyFlags=deny, returnStats=True, bits=8)
    print(dims, metric, deny, st)
    assert st["route"] == 1 and st["passes"] == 2
    check(eng, metric, queries[:5], d64, np.flatnonzero((flags & deny) == 0), 10, deny, got)
    assert st["certified"] == 5 and st["rerun"] == 0, st
    assert deny != OUTSIDE or st["tiles_skipped"] > 0


@pytest.mark.parametrize("metric", [COS, DOT])
@pytest.mark.parametrize("dims", [512, 1024, 1536])
def test_every_k_step_and_tile_position_counts(wax, dims, metric):
    """Query s is +-1 on the 64 elements of k-step s and zero elsewhere; rows 16 (3 + s) + p, p = 0, 5, 15, are that pattern times
    1.0, 0.8, 0.6 over noise of norm 0.3: the query's three best rows, in that order, far apart (cosine 0.96, 0.94, 0.89). 2 400 rows,
    so that the 128 candidates are chosen by key: a dropped, doubled or mispaired piece of K, or a wrong digit column, gives a
    planted row the key of a noise row and it is lost. One call of D / 64 <= 24 queries."""
    ksteps, rng = dims // 64, np.random.default_rng(dims + metric)
    corpus = 0.3 * unit_rows(2400, dims, dims + 7)
    queries = np.zeros((ksteps, dims), dtype=np.float32)
    for s in range(ksteps):
        queries[s, 64 * s:64 * s + 64] = rng.choice([-1.0, 1.0], 64) / 8.0
        for p, w in ((0, 1.0), (5, 0.8), (15, 0.6)):
            corpus[16 * (3 + s) + p] += np.float32(w) * queries[s]
    eng, _ = make_engine(wax, corpus, metric)
    *got, st = eng.searchMirror(queries, 3, returnStats=True, bits=8)
    check(eng, metric, queries, distances64(corpus, queries, metric), np.arange(2400), 3, 0, got)
    assert np.array_equal(got[0], ID0 + 16 * (3 + np.arange(ksteps))[:, None] + np.array([0, 5, 15])[None, :])
    assert st["route"] == 1 and st["certified"] == ksteps and st["rerun"] == 0, st


def test_follows_an_append_and_a_removal(wax):
    corpus, queries = unit_rows(1500, 1024, 21), unit_rows(5, 1024, 22)
    eng, _ = make_engine(wax, corpus, COS)
    new = unit_rows(37, 1024, 23)
    new[11] = queries[2]                                             # the new best hit of query 2
    first = eng.searchArrays(queries[0], 1)[0]
    steps = [lambda: None,
             lambda: eng.addBatch(np.arange(37, dtype=np.uint64) + ID0 + 5000, new),
             lambda: eng.removeBatch(np.concatenate([first, np.arange(700, 720, dtype=np.uint64) + ID0]))]   # a former hit among them
    for step in steps:
        step()
        ids, scores, counts, st = eng.searchMirror(queries, 10, returnStats=True, bits=8)
        assert st["route"] == 1 and st["passes"] == 2 and st["certified"] == 5 and st["rerun"] == 0, st
        for q in range(5):
            e_ids, e_scores = eng.searchArrays(queries[q], 10)
            assert counts[q] == 10 and np.array_equal(ids[q], e_ids) and np.array_equal(scores[q], e_scores), (eng.count, q)
    assert ids[2, 0] == ID0 + 5011 and first[0] not in ids[0]


@pytest.mark.parametrize("case", ["dims384", "l2", "k17"])
def test_forwarded_shapes_return_the_existing_search(wax, case):
    dims, k = (384, 10) if case == "dims384" else (1024, 17 if case == "k17" else 10)
    eng, _ = make_engine(wax, unit_rows(300, dims, 31), L2 if case == "l2" else COS)
    queries = unit_rows(5, dims, 32)
    ids, scores, counts, st = eng.searchMirror(queries, k, returnStats=True, bits=8)
    assert st["route"] == 0 and st["passes"] == 0
    for q in range(5):
        e_ids, e_scores = eng.searchArrays(queries[q], k)
        assert counts[q] == len(e_ids) == k and np.array_equal(ids[q, :k], e_ids) and np.array_equal(scores[q, :k], e_scores)


def test_the_default_is_still_the_bf16_mirror(store):
    eng, _, queries, d64 = store(512, COS, 4097)
    eng.searchMirror(queries, 10, bits=8)
    *got, st = eng.searchMirror(queries, 10, returnStats=True)
    assert "chunks_skipped" in st and "candidates" not in st and st["route"] == 1 and st["passes"] == 3 and st["certified"] == 9
    check(eng, COS, queries, d64, np.arange(4097), 10, 0, got)
