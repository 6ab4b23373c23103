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


# ---------------------------------------------------------------------------
# What test_mirror8_edges_gpu.py stands on: the f64 checks accept an IEEE f32 quantiser and refuse a subtly wrong one, and each
# construction has the property that lets its GPU test fail.

def edge_stores():
    for name, x, metric in constructions(R.queries_for(384)[0]):
        if name != "clustered":
            yield name, x, metric
    yield "inf / NaN / zero block, cosine", R.non_finite_store(0), 0
    yield "inf / NaN / zero block, dot", R.non_finite_store(1), 1
    yield "subnormal / huge / flat, dot", R.extreme_dot_store(), 1


@pytest.fixture(scope="module")
def dot384():
    x = R.corpus_for(1, 20005, 384)
    return x, R.Coded(x, 1)


def test_f64_checks_accept_an_ieee_quantiser_on_every_store():
    """quantise() divides and rounds in f32 as the kernel does (correctly rounded division): its codes, scale and err pass every check
    the GPU file applies to the device's, on every store it applies them to — so a failure there is the kernel's."""
    for name, x, metric in edge_stores():
        c = R.Coded(x, metric)
        classes = R.check_rows(x, metric, R.to_bytes(c.codes), c.scale, c.err, name)
        assert sum(classes.values()) == len(x), name
        want = R.expected_max_norm(x)
        assert want is not None and (np.isinf(want) or abs(want - c.max_norm) < 1e-12), name


def test_a_flat_code_tolerance_is_not_what_f32_division_gives(dot384):
    """Why check_rows lets a code sit 0.5 + (|code| + 1) 2^-24 units from its element rather than a flat 0.5 + 2^-20: the code is
    rint of the f32 quotient, and a quotient near 100 carries up to 2^-18 of rounding. The IEEE quantiser itself has elements beyond
    0.5 + 2^-20 on the Gaussian dot store, and none beyond the bound used."""
    x, c = dot384
    units = np.abs(c.scale.astype(np.float64)[:, None] * c.codes - x.astype(np.float64)) / c.scale.astype(np.float64)[:, None]
    assert np.sum(units > 0.5 + 2.0 ** -20) >= 1 and np.all(units <= 0.5 + (np.abs(c.codes) + 1.0) * 2.0 ** -24)


def test_f64_checks_refuse_a_subtly_wrong_mirror(dot384):
    x, c = dot384
    b = R.to_bytes(c.codes)
    R.check_rows(x, 1, b, c.scale, c.err, "as built")
    for what, args in {
        "no bound": (b, c.scale, c.err * np.float32(0.5)),                                    # an err half what it should be
        "no bound ": (b, c.scale, c.err * np.float32(1.0 - 2e-4)),                              # ... or short by two parts in 10^4 (D 2^-23 is 5e-5)
        "loose": (b, c.scale, c.err * np.float32(2.0)),
        "loose ": (b, c.scale, c.err * np.float32(1.0 + 3e-4)),
        "not the rounded": (b.reshape(len(b), -1, 4)[:, :, [1, 0, 2, 3]].reshape(b.shape), c.scale, c.err),   # two bytes of every dword swapped
        "not the rounded ": (np.where(np.arange(384) == 5, b + (b < 255), b).astype(np.uint8), c.scale, c.err),  # one element truncated, not rounded
        "scale of rows": (b, c.scale * np.float32(1.0 + 1e-6), c.err),
        "byte 0": (np.where(np.arange(384) == 0, 0, b).astype(np.uint8), c.scale, c.err),
    }.items():
        with pytest.raises(AssertionError, match=what.strip()):
            R.check_rows(x, 1, *args, what)
    part = c.err.copy()                                                                        # err summed over half of the wave, on one row
    half = c.scale[77].astype(np.float64) * c.codes[77, :192] - x[77, :192].astype(np.float64)
    part[77] = np.float32(np.sqrt(np.sum(half * half)))
    with pytest.raises(AssertionError, match="no bound on rows \\[77\\]"):
        R.check_rows(x, 1, b, c.scale, part, "partial sum")
    stale = b.copy()
    stale[100] = b[101]                                                                        # a code row left behind by a compaction
    with pytest.raises(AssertionError, match="not the rounded"):
        R.check_rows(x, 1, stale, c.scale, c.err, "stale row")
    with pytest.raises(AssertionError, match="max-norm word"):
        R.check_max_norm(x, c.max_norm * (1 + 1e-4))
    with pytest.raises(AssertionError, match="max-norm word"):
        R.check_max_norm(x, np.inf)
    R.check_max_norm(x, np.float32(c.max_norm))


def test_extreme_dot_rows_leave_the_range_of_f32_squares():
    """The rows do what extreme_dot_store says: in plain f32 the squared rounding differences of the subnormal rows sum to 0 and
    those of the 1e21 rows to +inf, while the err they ask for is an ordinary f32; the 1e19 rows have a norm beyond f32."""
    x = R.extreme_dot_store()
    c = R.Coded(x, 1)
    assert np.all(np.isfinite(c.err)) and np.all(c.err > 0) and np.all(np.isfinite(c.scale))
    with np.errstate(all="ignore"):
        diff = (c.scale[:, None] * c.codes.astype(np.float32) - x).astype(np.float32)
        naive = np.sum(diff * diff, axis=1, dtype=np.float32)
        norm2 = np.sum(x * x, axis=1, dtype=np.float32)
    sub, huge, huger = R.EXTREME_SUBNORMAL, R.EXTREME_HUGE, R.EXTREME_HUGER
    assert np.all(np.abs(x[sub]) < np.finfo(np.float32).tiny) and np.all(naive[sub] == 0) and np.all(c.err[sub] > 100 * R.TINY)
    assert np.all(np.isinf(norm2[huge])) and np.all(np.isfinite(naive[huge]))
    assert np.all(np.isinf(naive[huger])) and np.all(c.err[huger] < 1e21)
    assert set(np.unique(c.codes[R.EXTREME_FLAT])) == {-127, 127}
    assert np.isinf(R.expected_max_norm(x))


@pytest.mark.parametrize("appended", [False, True], ids=["bulk", "appended"])
@pytest.mark.parametrize("metric", [0, 1], ids=["cosine", "dot"])
@pytest.mark.parametrize("dims", [384, 768])
def test_aligned_row_is_a_candidate_only_through_its_err(dims, metric, appended):
    """With err A is the first of the 64 candidates; without it A is not among them, and the certificate computed without err would
    pass for k = 1 and 5 — a kernel that loses err returns a wrong top-1 on this store, certified. With err neither k certifies, by
    far more than a slack."""
    x, a, at = R.aligned_store(dims, metric, appended)
    if appended:
        x, at = np.vstack([x, a[None, :]]), len(x)
    q = R.aligned_query(a, metric)
    c = R.Coded(x, metric)
    assert c.err[at] > 8 * np.median(c.err)
    order = np.argsort(R.lower_bounds(q, c.codes, c.scale, c.err, metric), kind="stable")
    assert order[0] == at
    bare = R.lower_bounds(q, c.codes, c.scale, np.zeros_like(c.err), metric)
    order = np.argsort(bare, kind="stable")
    assert at not in order[:R.KP] and int(np.flatnonzero(order == at)[0]) > 200
    d = np.sort(R.exact_distances(x[order[:R.KP]], q, metric))
    sl = R.slack(dims, metric, float(np.linalg.norm(q.astype(np.float64))), c.max_norm)
    exact = R.exact_distances(x, q, metric)
    assert np.argmin(exact) == at and np.sort(exact)[1] - exact[at] > 3e-3
    for k in (1, 5):
        assert bare[order[R.KP - 1]] - sl - d[k - 1] > 10 * sl           # the false certificate passes
        assert c.margin(q, k) < -10 * sl                                  # the true one does not


@pytest.mark.parametrize("metric", [0, 1], ids=["cosine", "dot"])
@pytest.mark.parametrize("dims", [384, 768])
def test_ladder_margins_change_sign_inside_k(dims, metric):
    """For every query: at most 3 of the 16 k inside |margin| <= slack, at least 4 certify, at least 4 do not, k = 1 (the filler)
    certifies — and a model whose err is half (or gone) disagrees with the true one on at least 4 of the k that are checked, so the
    GPU test fails if the device's err is."""
    x, queries = R.ladder_store(dims, metric)
    c = R.Coded(x, metric)
    halved, gone = R.Coded(x, metric), R.Coded(x, metric)
    halved.err, gone.err = c.err * np.float32(0.5), np.zeros_like(c.err)
    cases = R.ladder_expectations(c, queries)
    assert len(queries) == R.LADDER_QUERIES and len(cases) == len(queries) * R.MAX_K
    for i, q in enumerate(queries):
        mine = [(k, m, sl) for j, k, m, sl in cases if j == i]
        band = [k for k, m, sl in mine if abs(m) <= sl]
        print(f"{dims}-d metric {metric} query {i}: margins in slacks", " ".join(f"{m / sl:+.1f}" for _, m, sl in mine))
        assert len(band) <= 3 and sum(m > sl for _, m, sl in mine) >= 4 and sum(m < -sl for _, m, sl in mine) >= 4
        assert mine[0][1] > 10 * mine[0][2]
        for broken in (halved, gone):
            assert sum((broken.margin(q, k) > 0) != (m > 0) for k, m, sl in mine if abs(m) > sl) >= 4


@pytest.mark.parametrize("metric", [0, 1], ids=["cosine", "dot"])
@pytest.mark.parametrize("dims", [384, 768])
def test_scan_row_count_edges_are_decided_by_far_more_than_a_slack(dims, metric):
    counts = R.scan_edge_counts(dims)
    assert counts == ([1, 63, 64, 65] if dims == 384 else [1, 31, 32, 33, 63, 64, 65])
    queries = R.queries_for(dims, 4)
    for n in counts:
        c = R.Coded(R.corpus_for(metric, n, dims, seed=81), metric)
        sl = R.slack(dims, metric, 1.0 + 1e-6, c.max_norm)
        for q, k in list(zip(queries, (1, 5, 10, 16))) + [(queries[1], 5)]:
            m = c.margin(q, min(k, n))
            assert (m == -np.inf) if n < R.KP else (abs(m) > 10 * sl), (n, k, m)
