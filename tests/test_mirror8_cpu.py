"""The 8-bit code mirror's bound and certificate, on the CPU and on the very inputs test_mirror8_gpu.py uses (mirror8_ref.py restates
the quantiser; no engine code runs here). (a) the per-row error bounds what the codes can move a dot product by, row by row, on every
construction; (b) the certificate holds for every Gaussian query the GPU file asserts `mirror8_fallbacks == 0` on, and fails on the
duplicate corpus — so "zero uncertified" there is a property of the inputs, proved beside them."""
import numpy as np
import pytest

import mirror8_ref as R


@pytest.fixture(scope="module")
def q384():
    return R.queries_for(384)


def constructions(q):
    yield "gaussian 384 cosine", R.corpus_for(0, 20005, 384), 0
    yield "gaussian 384 dot", R.corpus_for(1, 20005, 384), 1
    yield "gaussian 768 cosine", R.corpus_for(0, 5003, 768), 0
    yield "gaussian 768 dot", R.corpus_for(1, 5003, 768), 1
    yield "clustered", R.clustered_store(q), 0
    yield "outlier element", R.outlier_store(), 0
    yield "zero rows", R.zero_row_store(), 0


def test_row_error_bounds_the_dot_product_row_by_row(q384):
    """(a) |q.v~ - q.x^| <= ||q|| err_r for every row (f64 on both sides: the f32 arithmetic of the scan is the slack's business)."""
    for name, x, metric in constructions(q384[0]):
        c = R.Coded(x, metric)
        assert np.all(np.isfinite(c.err)) and np.all(c.err >= 0), name
        for q in R.queries_for(x.shape[1], 4):
            q64 = q.astype(np.float64)
            moved = np.abs(R.approx_dots(q, c.codes, c.scale) - c.xhat.astype(np.float64) @ q64)
            assert np.all(moved <= np.linalg.norm(q64) * c.err.astype(np.float64)), name
        if name == "zero rows":
            assert np.all(c.scale[20:5000] == 0) and np.all(c.codes[20:5000] == 0) and np.all(c.err[20:5000] <= 1e-44)


def test_rows_that_cannot_be_coded_are_always_candidates(q384):
    x = R.corpus_for(0, 200, 384, seed=3).copy()
    x[7, 3] = np.inf
    x[9, 11] = np.nan
    for metric in (0, 1):
        c = R.Coded(x, metric)
        # cosine: a NaN norm makes the row a zero row (distance 1), as on the f32 scan; the inf row's elements become NaN. dot: both.
        lost = [7] if metric == 0 else [7, 9]
        assert np.all(np.isinf(c.err[lost])) and np.sum(np.isinf(c.err)) == len(lost)
        lb = R.lower_bounds(q384[0], c.codes, c.scale, c.err, metric)
        assert np.all(lb[lost] == -np.inf) and np.all(np.isfinite(np.delete(lb, lost)))
        if metric == 0:
            assert c.scale[9] == 0 and not c.codes[9].any() and abs(lb[9] - 1.0) < 1e-6


@pytest.mark.parametrize("metric", [0, 1], ids=["cosine", "dot"])
@pytest.mark.parametrize("shape", R.GAUSSIAN_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_certificate_holds_on_the_gaussian_stores(shape, metric):
    """(b) every query, k = 1 / 10 / 16 — the GPU file asserts zero fallbacks for k <= 10 on exactly these."""
    n, dims = shape
    c = R.Coded(R.corpus_for(metric, n, dims), metric)
    for k in (1, 10, R.MAX_K):
        margins = [c.margin(q, k) for q in R.queries_for(dims)]
        print(f"{n}x{dims} metric {metric} k={k}: smallest margin {min(margins):.5f}")
        assert min(margins) > 0


def test_certificate_fails_where_the_gpu_file_expects_a_fallback(q384):
    q = q384[0]
    dup = R.Coded(R.duplicate_store(q), 0)
    assert all(not dup.margin(q, k) > 0 for k in (1, 10, R.MAX_K))          # 2 048 rows at the target's distance: 64 candidates cannot settle it
    clu = R.Coded(R.clustered_store(q), 0)
    assert all(not clu.margin(p, 10) > 0 for p in q384)                    # every query: the breaker's corpus
    nq = q.copy()
    nq[3] = np.nan
    assert not R.Coded(R.corpus_for(0, 5000, 384, seed=43), 0).margin(nq, 10) > 0


def test_outlier_row_is_a_candidate_and_the_others_still_certify(q384):
    c = R.Coded(R.outlier_store(), 0)
    typical = float(np.median(c.err))
    assert c.err[R.OUTLIER_ROW] > 3 * typical and np.max(np.delete(c.err, R.OUTLIER_ROW)) < 2 * typical
    for q in q384:
        lb = R.lower_bounds(q, c.codes, c.scale, c.err, 0)
        assert R.OUTLIER_ROW in np.argsort(lb, kind="stable")[:R.KP]
        assert c.margin(q, 10) > 0


def test_zero_rows_certify(q384):
    c = R.Coded(R.zero_row_store(), 0)
    assert all(c.margin(q, 10) > 0 for q in q384)
