"""The query of the 8-bit pass as three int8 digits per element (mirror8_planes_ref.py restates the kernel's quantiser): the digits
fit and recombine exactly, the quantised query is within delta sqrt(D) / 2 of the query, and the sum the matrix pipe computes stays
inside ||q|| err + term (a) of the slack of the exact product — on the seeded stores and queries of test_mirror_pass_forms_gpu.py,
both metrics, 384-d and 768-d, and on queries chosen against a quantiser scaled by max|q|. It also shows that every (store, query,
k) of test_mirror8_mfma_gpu.py's end-to-end test certifies with a margin above the floor: zero fallbacks there are a condition."""
import numpy as np
import pytest

import mirror8_planes_ref as P
import mirror8_ref as R8
import predicate_mirror_ref as R16


def check_query(q, cd, ctx):
    dims = q.size
    m, delta = P.quantise(q)
    a, b, c = P.digits(m)
    for name, d in (("a", a), ("b", b), ("c", c)):
        assert d.min() >= -64 and d.max() <= 63, f"{ctx}: digit {name} leaves [-64, 63]: {d.min()} .. {d.max()}"
    assert np.array_equal(16384 * a + 128 * b + c, m), f"{ctx}: the digits do not recombine"
    assert np.abs(m).max() <= P.M
    q64 = q.astype(np.float64)
    qhat = float(delta) * m.astype(np.float64)
    qn = float(np.linalg.norm(q64))
    moved = float(np.linalg.norm(qhat - q64))
    print(f"{ctx}: delta {float(delta):.3e}, ||q^ - q|| / ||q|| = {moved / qn if qn > 0 else 0.0:.3e}, bound {float(delta) * np.sqrt(dims) / 2 / qn if qn > 0 else 0.0:.3e}")
    assert moved <= float(delta) * np.sqrt(dims) / 2.0, f"{ctx}: ||q^ - q|| = {moved} > delta sqrt(D) / 2"
    # the sum of the quantised form against the exact product with the rows the codes approximate
    S = P.integer_sums(cd.codes, m).astype(np.float64)
    approx = float(delta) * cd.scale.astype(np.float64) * S
    ok = np.isfinite(cd.err)
    exact = cd.xhat[ok].astype(np.float64) @ q64
    vn = 1.0 if cd.metric == 0 else cd.max_norm
    bound = qn * cd.err[ok].astype(np.float64) + P.term_a(dims, qn, vn)
    gap = np.abs(approx[ok] - exact)
    worst = int(np.argmax(gap - bound))
    assert np.all(gap <= bound), f"{ctx}: row {worst}: |delta scale S - q.x^| = {gap[worst]} > ||q|| err + term (a) = {bound[worst]}"


@pytest.mark.parametrize("metric,dims", P.CASES, ids=P.CASE_IDS)
def test_the_digits_fit_recombine_and_keep_the_sum_inside_the_slack(metric, dims):
    cd = P.coded(metric, dims)
    for i, q in enumerate(P.queries(dims)):
        check_query(q, cd, f"metric {metric} dims {dims} query {i}")
    for name, q in P.adversarial_queries(dims).items():
        if name in P.NON_FINITE:
            continue
        check_query(q, cd, f"metric {metric} dims {dims} {name}")


def test_two_thousand_random_queries_quantise_within_the_bound():
    rng = np.random.default_rng(89)
    worst = 0.0
    for i in range(2000):
        dims = (384, 768)[i & 1]
        q = rng.standard_normal(dims).astype(np.float32) * np.float32(10.0 ** rng.uniform(-3, 3))
        if i % 5 == 0:
            q[rng.integers(dims)] *= np.float32(rng.uniform(5, 200))      # a dominant element
        m, delta = P.quantise(q)
        a, b, c = P.digits(m)
        assert min(a.min(), b.min(), c.min()) >= -64 and max(a.max(), b.max(), c.max()) <= 63
        assert np.array_equal(16384 * a + 128 * b + c, m)
        q64 = q.astype(np.float64)
        moved = np.linalg.norm(float(delta) * m - q64)
        assert moved <= float(delta) * np.sqrt(dims) / 2.0
        worst = max(worst, moved / np.linalg.norm(q64) * np.sqrt(384.0 / dims))
    print(f"worst ||q^ - q|| / ||q||, scaled to 384-d: {worst:.3e}")
    assert worst <= 9.42e-6         # delta sqrt(384) / 2 <= 9.42e-6 ||q||, since max|q| <= ||q||


@pytest.mark.parametrize("dims", [384, 768])
def test_queries_that_are_not_finite_or_null_never_divide_and_never_certify(dims):
    cd = P.coded(0, dims)
    adv = P.adversarial_queries(dims)
    for name in P.NON_FINITE:
        m, delta = P.quantise(adv[name])
        assert np.isnan(delta) and not m.any()
        keys = P.keys64(adv[name], cd.codes, cd.scale, cd.err, 0)
        assert np.all(np.isneginf(keys)), f"{name}: a key is finite, so the 64th could certify"
        assert P.margin(cd, adv[name], 1) == -np.inf
    m, delta = P.quantise(adv["all zero"])
    assert delta == 0 and not m.any()
    keys = P.keys64(adv["all zero"], cd.codes, cd.scale, cd.err, 0)
    assert np.all(np.isfinite(keys)) and np.allclose(keys, 1.0 - cd.err)       # s = 0: the null query's rule


@pytest.mark.parametrize("metric,dims", P.CASES, ids=P.CASE_IDS)
def test_every_store_query_and_k_of_the_gpu_test_certifies_with_margin(metric, dims):
    cd = P.coded(metric, dims)
    qs = P.queries(dims)
    margins = [P.margin(cd, q, k) for i, q in enumerate(qs) for k in (1, P.mixed_k(i), R8.MAX_K)]
    print(f"metric {metric} dims {dims}: smallest margin of the quantised form {min(margins):.5f}")
    assert min(margins) > R16.MARGIN_FLOOR


@pytest.mark.parametrize("dims", [384, 768])
def test_the_layout_data_is_exact_in_24_bits(dims):
    x, q = P.layout_store(P.N, dims), P.layout_query(dims)
    assert len({row.tobytes() for row in x}) == P.N, "two rows are equal"
    assert len(set(q.tolist())) == dims, "two query elements are equal"
    m, delta = P.quantise(q)
    assert delta == 1.0 and np.array_equal(m, q.astype(np.int64))
    a, b, c = P.digits(m)
    assert a.any() and b.any() and c.any() and a[0] == 63
    codes, scale, err = R8.quantise(R8.normalise(x, 1))
    assert np.all(scale == 1.0) and np.array_equal(codes, x.astype(np.int16))
    S = P.integer_sums(codes, m)
    assert np.abs(S).max() < 2 ** 24 - 1 and len(set(S.tolist())) > P.N // 2
    for plane in (a, b, c):
        assert np.abs(P.integer_sums(codes, plane)).max() < 2 ** 24
