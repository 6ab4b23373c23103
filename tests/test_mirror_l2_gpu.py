"""searchMirrorL2 ("L2 on the bf16 mirror"): L2 queries answered from shared passes over the bf16 mirror, certified in f32.
Every answer is held bit for bit to the engine's own search (searchArrays; searchFiltered under a predicate) and its ids to a plain
float64 reference, ((V - q)^2).sum(1) with ties by row.

Rows and queries are Gaussian directions with norms uniform in 0.5 .. 1, so L2 ranks differently from cosine and dot. On that corpus
a numpy model of the key (64 queries at each of the sizes below) keeps |key - d| below 7.2e-4 against an eps of 2.0e-3 .. 4.1e-3, and
a_64 - eps - d_k is at least 0.0095 at k = 10, so k <= 10 on 257 rows or more must certify; at k = 32 (at least 0.0016 in the model:
thin beside the f32 roundings the model leaves out) a re-run is allowed."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
COS, DOT, L2 = 0, 1, 2
ID0 = 1000            # frame id of row 0
# flag bits: a random half; rows outside one contiguous sixteenth; every row; every row but one; one row alone
HALF, OUTSIDE, ALL, ALL_BUT_ONE, ONE_ROW = 0x100, 0x200, 0x400, 0x800, 0x1000
MASKS = {"half": HALF, "sixteenth": OUTSIDE, "none": ALL, "one": ALL_BUT_ONE, "all_but_one": ONE_ROW}


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


def make_engine(wax, corpus, metric=L2, one_row=0, **kw):
    n = len(corpus)
    eng = wax.HIPVectorEngine(metric=wax.VectorMetric(metric), dimensions=corpus.shape[1], **kw)
    ids = np.arange(n, dtype=np.uint64) + ID0
    eng.addBatch(ids, corpus)
    flags = np.where(np.random.default_rng(n).random(n) < 0.5, HALF, 0).astype(np.uint32) | ALL | ALL_BUT_ONE | OUTSIDE
    flags[n // 2:n // 2 + n // 16] &= ~np.uint32(OUTSIDE)
    flags[n // 3] &= ~np.uint32(ALL_BUT_ONE)
    flags[one_row] |= ONE_ROW
    eng.setAttributes(ids, np.arange(n, dtype=np.int64), flags)
    return eng, flags


@pytest.fixture(scope="module")
def store(wax):
    """(dims, rows) -> engine, flags, nine queries and their float64 distances to every row; built once."""
    cache = {}

    def get(dims, n):
        if (dims, n) not in cache:
            corpus, queries = shell_rows(n, dims, 11 + dims + n), shell_rows(9, dims, 5 + dims)
            v64 = corpus.astype(np.float64)
            d64 = np.stack([((v64 - q) ** 2).sum(1) for q in queries.astype(np.float64)])
            # ONE_ROW marks query 0's best row: denying it takes one row out of an otherwise live chunk, and out of that answer
            cache[dims, n] = make_engine(wax, corpus, one_row=int(np.argmin(d64[0]))) + (queries, d64)
        return cache[dims, n]
    return get


def reference_ids(d64_q, rows, k):
    return ID0 + rows[np.lexsort((rows, d64_q[rows]))[:k]]


@pytest.mark.parametrize("k", [1, 10, 32])
@pytest.mark.parametrize("nq", [1, 2, 3, 4, 9])
@pytest.mark.parametrize("n", [15, 257, 4097, 40001])
@pytest.mark.parametrize("dims", [384, 768])
def test_equals_the_f32_scan_and_the_float64_reference(store, dims, n, nq, k):
    eng, _, queries, d64 = store(dims, n)
    ids, scores, counts, st = eng.searchMirrorL2(queries[:nq], k, stats=True)
    assert st["route"] == 1 and st["passes"] == (nq + 3) // 4 and st["certified"] + st["rerun"] == nq and st["lists"] >= 1
    for q in range(nq):
        s_ids, s_scores = eng.searchArrays(queries[q], k)
        m = min(k, n)
        assert counts[q] == m == len(s_ids)
        assert np.array_equal(ids[q, :m], s_ids) and np.array_equal(scores[q, :m], s_scores), q
        assert np.array_equal(s_ids, reference_ids(d64[q], np.arange(n), k)), q
    if k <= 10 and n >= 257:
        assert st["certified"] == nq and st["rerun"] == 0, st


@pytest.mark.parametrize("mask", sorted(MASKS))
@pytest.mark.parametrize("k", [10, 32])
@pytest.mark.parametrize("nq", [1, 4])
@pytest.mark.parametrize("n", [257, 4097])
@pytest.mark.parametrize("dims", [384, 768])
def test_masked_equals_the_predicate_search_and_the_float64_reference(store, dims, n, nq, k, mask):
    eng, flags, queries, d64 = store(dims, n)
    rows = np.flatnonzero((flags & MASKS[mask]) == 0)
    ids, scores, counts, st = eng.searchMirrorL2(queries[:nq], k, denyFlags=MASKS[mask], stats=True)
    assert st["route"] == 1 and st["certified"] + st["rerun"] == nq
    assert len(rows) == {"none": 0, "one": 1, "sixteenth": n // 16, "all_but_one": n - 1}.get(mask, len(rows))
    for q in range(nq):
        f_ids, f_scores = eng.searchFiltered(queries[q], k, denyFlags=MASKS[mask])
        m = min(k, len(rows))
        assert counts[q] == m == len(f_ids)
        assert np.array_equal(ids[q, :m], f_ids) and np.array_equal(scores[q, :m], f_scores), q
        assert np.array_equal(f_ids, reference_ids(d64[q], rows, k)), q
    if mask == "sixteenth" and n == 4097:
        assert st["chunks_skipped"] > 0 and (k > 10 or st["certified"] == nq)   # 256 passing rows: the pass itself answers k = 10
    if mask == "all_but_one" and k <= 10:
        assert st["certified"] == nq and st["rerun"] == 0, st                   # 256 rows or more pass: the unmasked margin holds


@pytest.mark.parametrize("kind", ["pairs", "copies", "cluster"])
def test_certificate_refuses_what_it_cannot_prove(wax, kind):
    """pairs: every row twice. Ties INSIDE the 64 candidates are settled by the exact re-score (distance, then row), so such a query
    may certify and must still be the scan's answer. copies: 70 copies of the best row — the 64th key equals the k-th distance.
    cluster: every row within 1e-4 of one point — every distance within 4e-4 of the others, far inside eps. Those two must re-run."""
    corpus = shell_rows(514, 384, 3)
    queries = shell_rows(4, 384, 4)
    if kind == "pairs":
        corpus[1::2] = corpus[0::2]
    elif kind == "copies":
        queries[0] = corpus[300] * np.float32(1.01)
        corpus[:70] = corpus[300]
    else:
        corpus = corpus[:1] + shell_rows(514, 384, 8) * np.float32(1e-4)
    eng, _ = make_engine(wax, corpus)
    nq = 1 if kind == "copies" else 4
    ids, scores, counts, st = eng.searchMirrorL2(queries[:nq], 10, stats=True)
    for q in range(nq):
        s_ids, s_scores = eng.searchArrays(queries[q], 10)
        assert counts[q] == 10 and np.array_equal(ids[q], s_ids) and np.array_equal(scores[q], s_scores)
    assert st["certified"] + st["rerun"] == nq and (kind == "pairs" or st["rerun"] == nq)


@pytest.mark.parametrize("deny", [0, HALF])
def test_follows_upserts_removals_and_a_capacity_doubling(wax, deny):
    eng, _ = make_engine(wax, shell_rows(300, 384, 21))
    queries = shell_rows(5, 384, 22)
    steps = [lambda: None,
             lambda: eng.addBatch(np.arange(40, dtype=np.uint64) * 7 + ID0, shell_rows(40, 384, 23)),        # existing ids: overwritten in place
             lambda: eng.removeBatch(np.arange(30, dtype=np.uint64) * 9 + ID0 + 3),
             lambda: eng.addBatch(np.arange(300, dtype=np.uint64) + ID0 + 5000, shell_rows(300, 384, 24))]   # 570 rows > the 512 reserved
    for step in steps:
        step()
        ids, scores, counts, st = eng.searchMirrorL2(queries, 10, denyFlags=deny, stats=True)
        assert st["route"] == 1
        for q in range(5):
            e_ids, e_scores = eng.searchFiltered(queries[q], 10, denyFlags=deny) if deny else eng.searchArrays(queries[q], 10)
            assert counts[q] == 10 and np.array_equal(ids[q], e_ids) and np.array_equal(scores[q], e_scores), (eng.count, q)


@pytest.mark.parametrize("case", ["cosine", "dims100", "k33", "sharded"])
def test_forwarded_shapes_return_the_existing_search(wax, case):
    dims, k = (100, 10) if case == "dims100" else (384, 33 if case == "k33" else 10)
    eng, _ = make_engine(wax, shell_rows(300, dims, 31), metric=COS if case == "cosine" else L2,
                         **({"devices": [0, 0, 0]} if case == "sharded" else {}))
    queries = shell_rows(5, dims, 32)
    for deny in (0, HALF):
        ids, scores, counts, st = eng.searchMirrorL2(queries, k, denyFlags=deny, stats=True)
        assert st["route"] == 0 and st["passes"] == 0
        for q in range(5):
            e_ids, e_scores = eng.searchFiltered(queries[q], k, denyFlags=deny) if deny else eng.searchArrays(queries[q], k)
            assert counts[q] == len(e_ids) == k and np.array_equal(ids[q, :k], e_ids) and np.array_equal(scores[q, :k], e_scores)
