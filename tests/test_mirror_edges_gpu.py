"""The bf16-mirror paths at the edges of their exactness argument: both certificates need
`approximate distance <= exact distance + eps` for EVERY row of the store. The rows and queries here are the ones for which that is
hardest to keep: rows the cosine rule scores 0 when they are the best rows of the store, rows whose norm sits on the 1e-6 rule,
the measured words of the bound after every kind of mutation, aligned rounding errors on the single-query path, magnitudes bf16
cannot hold. Every answer is held (a) to the engine's own f32 scan, bit for bit, and (b) to the f64 oracle / numpy.
The constructions are proved in tests/test_mirror_edges_cpu.py."""
import numpy as np
import pytest

import oracle
from helpers import (SCORE_TOL, OracleEngine, anti_correlated_corpus, assert_parity, bf16_adversarial_unit_vector, bf16_rne,
                     threshold_rows)

pytestmark = pytest.mark.gpu

ANTI_SEED = 101
THRESHOLD_SEED = 202
NQ = 32            # a batch the MFMA pipelines take


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


def make_sharded(wax, metric, dims, corpus):
    many = wax.HIPVectorEngine(metric=wax.VectorMetric(metric), dimensions=dims, devices=[0] * 3)
    many.setTuning("shard_min_mb", 0)
    many.addBatch(np.arange(len(corpus), dtype=np.uint64), corpus)
    assert many.shardCount == 3
    return many


COUNTERS = ("mirror_scans", "mirror_scan_fallbacks", "mirror_scan_unavailable", "batch_queries", "onepass_queries", "batch_fallbacks",
            "batch_retries", "batch_inline_retries")


def counters(eng):
    return {n: eng.getTuning(n) for n in COUNTERS}


def moved(before, after):
    return {n: after[n] - before[n] for n in COUNTERS if after[n] != before[n]}


def f32_scan(eng, q, k):
    eng.setTuning("scan_mirror", 0)
    return eng.searchArrays(q, k)


def nearby_queries(q, nq, seed, keep_zero=None):
    """q itself, q scaled, and unit vectors a few degrees away from q (component `keep_zero` stays exactly 0)."""
    rng = np.random.default_rng(seed)
    out = np.empty((nq, q.size), dtype=np.float32)
    out[0] = q
    out[1] = q * np.float32(3.0)
    for i in range(2, nq):
        g = rng.standard_normal(q.size)
        if keep_zero is not None:
            g[keep_zero] = 0.0
        v = q.astype(np.float64) + 0.02 * g / np.linalg.norm(g)
        out[i] = (v / np.linalg.norm(v)).astype(np.float32)
    return out


def check_against_oracle(metric, corpus, q, k, got, ctx):
    e_ids, e_scores, _, _ = oracle.search(metric, corpus, None, q, k + 16)
    n = min(k, len(e_ids))
    assert_parity(got[0], got[1], e_ids[:n], e_scores[:n], all_exp_scores=e_scores, ctx=ctx)


def single_mirror_answers(eng, queries, k, want, ctx, shards=1):
    """Every query through scan_mirror 2 — the counter shows the path was taken — equal to `want` (the f32 scan's) bit for bit."""
    eng.setTuning("scan_mirror", 2)
    before = counters(eng)
    got = [eng.searchArrays(q, k) for q in queries]
    after = counters(eng)
    assert after["mirror_scans"] - before["mirror_scans"] == shards * len(queries), (ctx, moved(before, after))
    assert after["mirror_scan_unavailable"] == before["mirror_scan_unavailable"], ctx
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]), \
            f"{ctx}: mirror path, query {i}, k={k}: {g[0][:8]} {g[1][:8]} != f32 scan {w[0][:8]} {w[1][:8]}; counters moved {moved(before, after)}"
    return moved(before, after)


def batch_answers(eng, queries, k, want, ctx, onepass):
    """searchBatch on the one-pass pipeline (onepass 1) or the slab pipeline (0) — confirmed by the counters — equal to `want`."""
    eng.setTuning("batch_onepass", onepass)
    before = counters(eng)
    ids, scores, counts = eng.searchBatch(queries, k)
    after = counters(eng)
    assert after["batch_queries"] - before["batch_queries"] == len(queries), (ctx, onepass, moved(before, after))
    assert after["onepass_queries"] - before["onepass_queries"] == (len(queries) if onepass else 0), (ctx, onepass, moved(before, after))
    for i, w in enumerate(want):
        c = int(counts[i])
        assert np.array_equal(ids[i, :c], w[0]) and np.array_equal(scores[i, :c], w[1]), \
            f"{ctx}: searchBatch onepass={onepass}, query {i}, k={k}: {ids[i, :c][:8]} {scores[i, :c][:8]} != f32 scan {w[0][:8]} {w[1][:8]}; counters moved {moved(before, after)}"
    eng.setTuning("batch_onepass", 1)
    return moved(before, after)


def dot_expected(corpus, q, k):
    """numpy f64 for the dot metric: rows whose product is not finite are dropped, the others ranked (distance asc, row asc);
    scores cast the way hits_to_results does it: the key's f32 distance 1 - dot, score = -distance. k + 16 entries."""
    with np.errstate(all="ignore"):
        d = corpus.astype(np.float64) @ q.astype(np.float64)
    dist = np.where(np.isfinite(d), 1.0 - d, np.inf).astype(np.float32)
    order = np.argsort(dist, kind="stable")[:k + 16]
    return order, -dist[order]


# ---------------------------------------------------------------------------
# 1. a top k whose similarities are not positive

def planted_store(dims):
    corpus, q = anti_correlated_corpus(20000, dims, ANTI_SEED, zero_at=17)
    neg = int(np.argmin(q))                       # a column where the query is negative
    zero_score = [3, 5, 10000, 19998, 19999]      # cosine: similarity exactly 0
    corpus[5, 40] = np.nan                        # NaN rows: low and high row numbers
    corpus[19998, 383] = np.nan
    corpus[10000] = 0.0                           # a zero row in the middle
    corpus[3] *= np.float32(1e-7)                 # rows of norm 1e-7: first and last
    corpus[19999] *= np.float32(1e-7)
    corpus[9000, neg] = np.inf                    # one +inf component
    corpus[15000, 17] = -np.inf                   # -inf where the query component is exactly 0
    return corpus, q, zero_score, [9000, 15000]


@pytest.mark.parametrize("dims", [384, 768])
def test_cosine_top_k_of_zero_similarity_rows(wax, dims):
    """All ordinary rows lie opposite the query (cosine <= -0.05), so the rows the rule `sqrt(m) > 1e-6 ? dot / sqrt(m) : 0` scores 0 —
    NaN rows, a zero row, rows of norm 1e-7 — are the BEST rows of the store. Parent commit: the mirror kept a NaN in a NaN row, the
    approximate distance was +inf against an exact 1.0, and the certificate passed without the row."""
    corpus, q, zero_score, inf_rows = planted_store(dims)
    eng = make_engine(wax, 0, dims, corpus)
    many = make_sharded(wax, 0, dims, corpus)
    queries = nearby_queries(q, NQ, 7, keep_zero=17)
    report = {}
    for k in (1, 10, 32):
        want = [f32_scan(eng, qq, k) for qq in queries]
        # the pinned side itself, against the oracle and against the expectation spelled out
        for i in (0, 1, 2, NQ - 1):
            check_against_oracle(0, corpus, queries[i], k, want[i], f"f32 scan dims {dims} k {k} query {i}")
        top = min(k, len(zero_score))
        assert want[0][0][:top].tolist() == zero_score[:top] and np.all(want[0][1][:top] == 0.0)
        assert np.all(want[0][1][top:] <= -0.05 + SCORE_TOL) and not set(inf_rows) & set(want[0][0].tolist())
        report[("mirror", k)] = single_mirror_answers(eng, queries[:6], k, want[:6], f"dims {dims}")
        report[("onepass", k)] = batch_answers(eng, queries, k, want, f"dims {dims}", 1)
        report[("slab", k)] = batch_answers(eng, queries, k, want, f"dims {dims}", 0)
        report[("3 shards", k)] = single_mirror_answers(many, queries[:6], k, want[:6], f"3 shards dims {dims}", shards=3)
    print(f"dims {dims}: counters moved per path", report)
    eng.close()
    many.close()


@pytest.mark.parametrize("dims", [384, 768])
def test_dot_on_the_same_planted_rows(wax, dims):
    """Dot metric over the same store: a NaN row (and an inf component against a zero query component) has a NaN distance and is
    dropped; the zero row (dot 0) and the tiny rows are the best rows of the store."""
    corpus, q, _, inf_rows = planted_store(dims)
    eng = make_engine(wax, 1, dims, corpus)
    many = make_sharded(wax, 1, dims, corpus)
    queries = nearby_queries(q, NQ, 7, keep_zero=17)
    dots = corpus.astype(np.float64) @ q.astype(np.float64)
    dropped = set(np.flatnonzero(~np.isfinite(dots)).tolist())
    assert dropped == {5, 19998, 9000, 15000}
    report = {}
    for k in (1, 10, 32):
        want = [f32_scan(eng, qq, k) for qq in queries]
        for i in (0, 1, 2, NQ - 1):
            e_rows, e_scores = dot_expected(corpus, queries[i], k)
            assert_parity(want[i][0], want[i][1], e_rows[:k], e_scores[:k], all_exp_scores=e_scores, ctx=f"f32 scan dot dims {dims} k {k} query {i}")
        top = min(k, 3)                                # dot 0 (the zero row) and -1e-7 * 0.05 (the tiny rows): distance 1.0f, score -1.0
        assert want[0][0][:top].tolist() == [3, 10000, 19999][:top] and np.all(want[0][1][:top] == -1.0)
        assert not dropped & set(want[0][0].tolist()) and np.all(np.isfinite(want[0][1]))
        report[("mirror", k)] = single_mirror_answers(eng, queries[:6], k, want[:6], f"dot dims {dims}")
        report[("onepass", k)] = batch_answers(eng, queries, k, want, f"dot dims {dims}", 1)
        report[("slab", k)] = batch_answers(eng, queries, k, want, f"dot dims {dims}", 0)
        report[("3 shards", k)] = single_mirror_answers(many, queries[:6], k, want[:6], f"dot 3 shards dims {dims}", shards=3)
    print(f"dot dims {dims}: counters moved per path", report)
    # the count: everything but the dropped rows (a store small enough to ask for all of it)
    sel = np.concatenate([np.arange(1000), [9000, 10000, 15000, 19998, 19999]])
    small = make_engine(wax, 1, dims, corpus[sel], ids=sel.astype(np.uint64))
    ids, scores = small.searchArrays(q, len(sel))
    assert len(ids) == len(sel) - len(dropped) and not dropped & set(ids.tolist()) and np.all(np.isfinite(scores))
    eng.close()
    many.close()
    small.close()


# ---------------------------------------------------------------------------
# 2. rows whose norm sits on the 1e-6 rule

def threshold_store(dims):
    q = oracle.gaussian_unit_queries(1, dims)[0]
    corpus = oracle.gaussian_unit_rows(300, 20000, dims)
    rows, cosines, j = threshold_rows(q, 256, dims, THRESHOLD_SEED)
    where = 37 + 78 * np.arange(256)
    corpus[where] = rows
    return np.ascontiguousarray(corpus), q, where, j


def check_threshold_answer(corpus, q, k, got, where, j, ctx):
    """The f64 side of the threshold test. A returned row that is not a constructed row: the oracle's score within 1e-5. A returned
    constructed row: its true cosine within 1e-5 or exactly 0.0 (which side of 1e-6 the f32 sum falls on is not decidable in f64).
    Nothing better was left out. Returns the constructed rows that took the relaxed rule."""
    ids, scores = got
    assert len(ids) == k and np.all(np.diff(scores) <= 0), ctx
    o_scores = oracle.scores_from_distances(0, oracle.distances(0, corpus, q)).astype(np.float64)
    c64 = (corpus.astype(np.float64) @ q.astype(np.float64)) / (np.linalg.norm(corpus.astype(np.float64), axis=1) * np.linalg.norm(q.astype(np.float64)))
    constructed = set(where.tolist())
    relaxed = set()
    for r, s in zip(ids.tolist(), scores.tolist()):
        if r in constructed:
            assert abs(s - c64[r]) <= SCORE_TOL or s == 0.0, (ctx, r, s, c64[r])
            relaxed.add(r)
        else:
            assert abs(s - o_scores[r]) <= SCORE_TOL, (ctx, r, s, o_scores[r])
    out = np.ones(len(corpus), dtype=bool)
    out[ids.astype(np.int64)] = False
    clear = out.copy()
    clear[where[np.abs(j) < 8]] = False            # constructed rows within 8 steps of the rule may be on either side
    bound = float(scores[-1]) + SCORE_TOL
    assert not np.any(o_scores[clear] > bound), (ctx, np.flatnonzero(clear & (o_scores > bound))[:8])
    return relaxed


@pytest.mark.parametrize("dims", [384, 768])
def test_rows_on_the_norm_threshold(wax, dims):
    """256 rows of norm 1e-6 * (1 + j * 2^-24), cosines 0.955 ... 0.700 to the query, in a Gaussian corpus whose best cosine is
    about 0.25: the valid ones ARE the top k. The mirror has to call a row valid exactly when the f32 scan does."""
    corpus, q, where, j = threshold_store(dims)
    eng = make_engine(wax, 0, dims, corpus)
    many = make_sharded(wax, 0, dims, corpus)
    queries = nearby_queries(q, NQ, 11)
    allow = where.astype(np.uint64)
    relaxed = set()
    report = {}
    for k in (1, 10, 32):
        want = [f32_scan(eng, qq, k) for qq in queries]
        for i in (0, 1, 2, NQ - 1):
            relaxed |= check_threshold_answer(corpus, queries[i], k, want[i], where, j, f"f32 scan dims {dims} k {k} query {i}")
        assert set(want[0][0].tolist()) <= set(where.tolist()) and np.all(want[0][1] > 0.6)     # the constructed rows are the top k
        report[("mirror", k)] = single_mirror_answers(eng, queries[:8], k, want[:8], f"dims {dims}")
        report[("onepass", k)] = batch_answers(eng, queries, k, want, f"dims {dims}", 1)
        report[("slab", k)] = batch_answers(eng, queries, k, want, f"dims {dims}", 0)
        report[("3 shards", k)] = single_mirror_answers(many, queries[:8], k, want[:8], f"3 shards dims {dims}", shards=3)
        eng.setTuning("scan_mirror", 0)
        eng.setTuning("force_general", 1)
        for i in range(4):
            g = eng.searchArrays(queries[i], k)
            assert np.array_equal(g[0], want[i][0]) and np.array_equal(g[1], want[i][1]), ("force_general", dims, k, i)
        eng.setTuning("force_general", 0)
        for i in range(4):
            g = eng.searchFiltered(queries[i], k, frameIds=allow)
            assert np.array_equal(g[0], want[i][0]) and np.array_equal(g[1], want[i][1]), ("searchFiltered", dims, k, i)
        ids, scores, counts = eng.searchBatchFiltered(queries, k, frameIds=[allow] * NQ)
        for i in range(NQ):
            c = int(counts[i])
            assert np.array_equal(ids[i, :c], want[i][0]) and np.array_equal(scores[i, :c], want[i][1]), ("searchBatchFiltered", dims, k, i)
    print(f"dims {dims}: counters moved per path", report, "relaxed rows", len(relaxed))
    assert relaxed <= set(where.tolist()) and len(relaxed) <= 256      # the relaxed rule cannot spread beyond the constructed rows
    eng.close()
    many.close()


# ---------------------------------------------------------------------------
# 3. the measured words of the bound against numpy

def true_words(metric, rows, dims):
    """(max ||v||, max ||x - bf16(x)||) in f64 over the rows the mirror can vouch for; x = the row, normalised in f32 for cosine.
    Rows whose norm is not finite or within 2^-20 of the 1e-6 rule are left out; cosine rows below the rule are zero rows."""
    r64 = rows.astype(np.float64)
    with np.errstate(all="ignore"):
        norms = np.linalg.norm(r64, axis=1)
    keep = np.isfinite(norms)
    if metric == 0:
        keep &= np.abs(norms / 1e-6 - 1.0) > 2.0 ** -20
        valid = keep & (norms > 1e-6)
        scale = (np.float32(1.0) / norms[valid].astype(np.float32)).astype(np.float32)
        x = (rows[valid] * scale[:, None]).astype(np.float32)
    else:
        x = rows[keep]
    err = np.linalg.norm(x.astype(np.float64) - bf16_rne(x).astype(np.float64), axis=1)
    return float(np.max(norms[keep])), float(np.max(err)) if len(err) else 0.0


def check_words(eng, metric, rows, dims, ctx, tight):
    qs = oracle.gaussian_unit_queries(NQ, dims, seed=5)
    before = eng.getTuning("batch_queries")
    eng.searchBatch(qs, 10)                                   # brings the mirror up to date with the store
    assert eng.getTuning("batch_queries") - before == NQ, ctx
    norm_word, err_word = eng.getTuning("batch_max_norm_e6") * 1e-6, eng.getTuning("batch_max_row_err_e9") * 1e-9
    norm64, err64 = true_words(metric, rows, dims)
    rel = (dims + 4) * 2.0 ** -24
    print(f"{ctx}: norm word {norm_word:.6f} f64 {norm64:.9f}; error word {err_word:.9f} f64 {err64:.12f}")
    assert norm_word >= norm64 * (1 - rel) - 1e-6, (ctx, "norm word unsound", norm_word, norm64)
    assert err_word >= err64 * (1 - rel) - 1e-9, (ctx, "error word unsound", err_word, err64)
    if tight:
        assert norm_word <= norm64 * (1 + rel) + 1e-6, (ctx, "norm word loose", norm_word, norm64)
        assert err_word <= err64 * (1 + rel) + 1e-9, (ctx, "error word loose", err_word, err64)


def words_corpus(kind, dims):
    n = 20000
    x = oracle.gaussian_unit_rows(500, n, dims)
    if kind == "dot":
        x = x * np.random.default_rng(507).uniform(0.5, 2.0, size=(n, 1)).astype(np.float32)
    elif kind == "adversarial":
        x[4321] = bf16_adversarial_unit_vector(dims)
    elif kind == "threshold":
        x = threshold_store(dims)[0]
    return np.ascontiguousarray(x, dtype=np.float32)


@pytest.mark.parametrize("dims", [384, 768])
@pytest.mark.parametrize("kind", ["gaussian", "dot", "adversarial", "threshold"])
def test_measured_words_after_a_full_conversion(wax, kind, dims):
    metric = 1 if kind == "dot" else 0
    corpus = words_corpus(kind, dims)
    eng = make_engine(wax, metric, dims, corpus)
    check_words(eng, metric, corpus, dims, f"{kind} dims {dims}", tight=True)
    eng.close()


@pytest.mark.parametrize("metric", [0, 1], ids=["cosine", "dot"])
def test_measured_words_follow_every_mutation(wax, metric):
    """the two words "still bound" the mirror after every incremental step. Each step plants a row that raises the true
    maximum (cosine: an adversarial unit vector that loses more to rounding than any row so far; dot: a row of larger norm and
    rounding error), so a step that forgot the words would leave them below the f64 figure. After deserialize everything is
    converted again and the words are tight again."""
    dims, n = 384, 20000
    corpus = words_corpus("dot" if metric else "gaussian", dims)
    eng = make_engine(wax, metric, dims, corpus)
    model = OracleEngine(metric, dims)
    model.ids, model.rows = list(range(n)), [r for r in corpus]
    fracs = iter([0.90, 0.92, 0.94, 0.96, 0.97, 0.98, 0.985])

    def worst():
        f = next(fracs)
        v = bf16_adversarial_unit_vector(dims, f, roll=int(f * 1000) % 300)
        return v if metric == 0 else (v * np.float32(2.0 + 2.0 * f)).astype(np.float32)    # dot: norms 3.8 ... 3.97, the error grows with them

    def put(fid, v):
        eng.addBatch(np.array([fid], dtype=np.uint64), v[None, :])
        model.addBatch([fid], [v])

    def check(step, tight=False):
        assert eng.count == model.count, step
        check_words(eng, metric, model.matrix(), dims, f"metric {metric}: {step}", tight)

    check("bulk addBatch", tight=True)
    put(777, worst())
    check("upsert of a mirrored row")
    v = worst()
    eng.add(10 ** 6, v)
    model.add(10 ** 6, v)
    check("staged single add")
    extra = oracle.gaussian_unit_rows(900, 15000, dims)
    extra[7000] = worst()
    fresh = np.arange(2 * 10 ** 6, 2 * 10 ** 6 + 15000, dtype=np.uint64)
    eng.addBatch(fresh, extra)                                # 20 001 + 15 000 rows: past the 32 768 the store held
    model.addBatch(fresh.tolist(), [r for r in extra])
    check("addBatch that grows capacity")
    put(900, worst())
    eng.remove(5)
    model.remove(5)
    check("remove (with an upsert waiting behind the removed row)")
    put(901, worst())
    gone = np.arange(2000, 3000, dtype=np.uint64)
    assert eng.removeBatch(gone) == 1000
    for fid in gone.tolist():
        model.remove(fid)
    check("removeBatch of 1 000 ids that spare the planted rows")
    assert eng.removeBatch(np.array([901, 4000, 4001], dtype=np.uint64)) == 3
    for fid in (901, 4000, 4001):
        model.remove(fid)
    check("removeBatch that takes the worst row")             # the word may stay where it was: monotone
    put(902, worst())
    other = make_engine(wax, metric, dims, words_corpus("adversarial" if metric == 0 else "dot", dims) * np.float32(1 if metric == 0 else 4))
    other.searchBatch(oracle.gaussian_unit_queries(NQ, dims, seed=5), 10)     # a mirrored engine with LARGER words than the blob's store
    other.deserialize(eng.serialize())
    eng.close()
    eng = other
    check("serialize -> deserialize into a mirrored engine", tight=True)
    eng.close()


# ---------------------------------------------------------------------------
# 4. aligned rounding errors on the single-query mirror path

def aligned_store(dims, with_a=True):
    n = 40_000
    rng = np.random.default_rng(8)
    corpus = oracle.gaussian_unit_rows(77, n, dims)
    a = bf16_adversarial_unit_vector(dims)
    if with_a:
        corpus[1234] = a
    for jj, dist in enumerate(np.linspace(0.0030, 0.0065, 300)):
        u = rng.standard_normal(dims)
        u -= (u @ a.astype(np.float64)) * a.astype(np.float64)
        u /= np.linalg.norm(u)
        t = np.sqrt(1.0 / (1.0 - dist) ** 2 - 1.0)
        v = a.astype(np.float64) + t * u
        corpus[2000 + jj] = (v / np.linalg.norm(v)).astype(np.float32)
    return corpus, a


@pytest.mark.parametrize("dims", [384, 768])
@pytest.mark.parametrize("upsert", [False, True], ids=["bulk", "upsert-after-conversion"])
def test_aligned_rounding_errors_on_the_single_query_mirror_path(wax, dims, upsert):
    """The store of test_certificate_bound_survives_aligned_rounding_errors: row A loses 2^-8 of every element to rounding, so the
    mirror puts A at distance 0.0077 from itself, behind 300 honest neighbours at 0.0030 - 0.0065. The answer to the query A is A,
    score 1 — with the measured bound, with the worst-case constant, and when A arrives by upsert into a converted mirror (then
    the measured word has to have followed the upsert)."""
    corpus, a = aligned_store(dims, with_a=not upsert)
    ids = np.arange(len(corpus), dtype=np.uint64) + 1
    eng = make_engine(wax, 0, dims, corpus, ids)
    batch = oracle.gaussian_unit_queries(NQ, dims, seed=9)
    batch[3] = a
    batch[17] = a
    if upsert:
        eng.setTuning("scan_mirror", 2)
        eng.searchArrays(batch[0], 5)                         # converts the mirror
        eng.searchBatch(batch, 5)
        assert eng.getTuning("mirror_conversions") >= 1
        eng.addBatch(np.array([1235], dtype=np.uint64), a[None, :])
        corpus = corpus.copy()
        corpus[1234] = a
    for measured in (1, 0):
        eng.setTuning("batch_eps_measured", measured)
        for k in (1, 5):
            want = f32_scan(eng, a, k)
            e_ids, e_scores, _, _ = oracle.search(0, corpus, ids, a, k + 16)
            assert_parity(want[0], want[1], e_ids[:k], e_scores[:k], all_exp_scores=e_scores, ctx=f"f32 scan, k {k}")
            info = single_mirror_answers(eng, [a], k, [want], f"dims {dims} measured {measured} upsert {upsert}")
            got = eng.searchArrays(a, k)
            assert got[0][0] == 1235 and abs(float(got[1][0]) - 1.0) < 1e-6, (dims, measured, k, got, info)
            if upsert:                                        # the batched path gets the upsert variant too
                wants = [f32_scan(eng, qq, k) for qq in batch]
                for onepass in (1, 0):
                    eng.setTuning("batch_onepass_tiles", 64 if onepass else 1024)
                    batch_answers(eng, batch, k, wants, f"dims {dims} measured {measured}", onepass)
                assert wants[3][0][0] == 1235 and wants[17][0][0] == 1235
    eng.close()


# ---------------------------------------------------------------------------
# 5. f32 magnitudes bf16 cannot hold (dot)

def test_magnitudes_bf16_cannot_hold(wax):
    """3.4e38 is a finite f32 and rounds to bf16 inf. Row P holds it where the query is exactly 0 (the exact product is 0, the
    mirror's is inf * 0 = NaN) and is the best row of the store; row R holds it against a query component of 1e-38 (an honest
    product of 3.4). The mirror cannot vouch for P: its error word becomes inf and no certificate may pass."""
    dims, n = 384, 20000
    rng = np.random.default_rng(61)
    corpus = oracle.gaussian_unit_rows(600, n, dims) * rng.uniform(0.5, 2.0, size=(n, 1)).astype(np.float32)
    corpus = np.ascontiguousarray(corpus, dtype=np.float32)
    q = oracle.gaussian_unit_queries(1, dims, seed=62)[0].copy()
    q[100] = 0.0
    q[200] = np.float32(1e-38)
    big = np.float32(3.4e38)
    p_row, r_row = 12345, 777
    corpus[p_row] = q * np.float32(5.0)
    corpus[p_row, 100] = big
    corpus[r_row, 200] = big
    assert np.isfinite(big) and np.isinf(bf16_rne(np.array([big]))[0])
    dots = corpus.astype(np.float64) @ q.astype(np.float64)
    assert np.all(np.isfinite(dots)) and np.argmax(dots) == p_row and np.argsort(-dots)[1] == r_row
    queries = nearby_queries(q, NQ, 63, keep_zero=100)
    queries[:, 200] = np.float32(1e-38)

    eng = make_engine(wax, 1, dims, corpus)
    for k in (1, 10):
        want = [f32_scan(eng, qq, k) for qq in queries]
        for i in (0, 2, NQ - 1):
            e_rows, e_scores = dot_expected(corpus, queries[i], k)
            assert_parity(want[i][0], want[i][1], e_rows[:k], e_scores[:k], all_exp_scores=e_scores, ctx=f"f32 scan k {k} query {i}")
            assert np.all(np.isfinite(want[i][1]))
        assert want[0][0][0] == p_row
        info = single_mirror_answers(eng, queries[:6], k, want[:6], f"k {k}")
        assert info.get("mirror_scan_fallbacks", 0) == 6, ("the mirror path certified an answer it cannot vouch for", info)
        for onepass in (1, 0):
            info = batch_answers(eng, queries, k, want, f"k {k}", onepass)
            assert info.get("batch_fallbacks", 0) + info.get("batch_retries", 0) + info.get("batch_inline_retries", 0) > 0, \
                ("the batched path certified every query of a store whose mirror holds a NaN row", onepass, info)
    eng.close()
