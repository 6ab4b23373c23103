"""The construction behind tests/test_batch_positions_gpu.py, proved on the host so that the GPU sweeps can fail (tests/batch_positions_ref.py).

For every store of the table: (a) every pair's float64 cosine lies in [0.90, 0.99] and the rows have one common norm, so the dot and L2
orders are the cosine order; (b) no stranger outranks a twin — directly, by a blocked matrix product, on the smallest store of each
dimension, and by the spherical-cap bound of batch_positions_ref.cap_bound on the others, summed over N^2 pairs at t = 0.8 and held
below 1e-3; (c) on at least 256 queries the 64th best approximate distance less the worst-case eps less the exact second distance
exceeds 0.3 (in units of the cosine distance), so a fallback of the sweep is never owed to the certificate — it can only come from a
survivor segment that overflowed or a threshold sampled too low; (d) a model filter that loses any one row position changes exactly two
answers of the sweep, that row's own and its twin's. And for every case: H is no multiple of the rows between two tiles of a
workgroup's share, the pool (where the case claims one) exists and has pairs on both of its sides, the query groups are what the case
says."""
import numpy as np
import pytest

import batch_positions_ref as P


def _smallest_per_dim():
    best = {}
    for metric, dims, n in P.stores():
        if dims not in best or n < best[dims][2]:
            best[dims] = (metric, dims, n)
    return set(best.values())


SMALLEST = _smallest_per_dim()


def test_the_table_has_the_cases_of_the_issue():
    by_route = {}
    for c in P.CASES:
        by_route.setdefault(c["route"], []).append((c["metric"], c["dims"], c["n"], c["nq"]))
    assert by_route[P.POOL] == [(P.COS, 384, 24 * 256 * 64 + 37, 256), (P.COS, 768, 24 * 256 * 32 + 19, 256)]
    assert by_route[P.FIXED] == [(P.COS, d, 40_037, 256) for d in (128, 256, 384, 512, 768)] + [(P.DOT, 384, 40_037, 256), (P.COS, 384, 4_099, 256)]
    assert by_route[P.GROUPS] == [(P.COS, d, 40_037, nq) for d in (384, 768) for nq in (512, 768, 1024)]
    assert by_route[P.SPLIT] == [(P.COS, 384, 40_037, 256), (P.COS, 768, 40_037, 256)]
    assert by_route[P.TILED] == [(P.COS, 64, 65_613, 256), (P.DOT, 192, 65_613, 256), (P.L2, 384, 65_613, 256)]
    assert by_route[P.SLAB] == [(P.COS, 384, 20_011, 256), (P.COS, 384, 20_011, 256), (P.COS, 384, 3_001, 256)]
    assert by_route[P.EXACT] == [(P.COS, 384, 5_003, 256), (P.L2, 100, 5_003, 256)]
    assert by_route[P.HANDLE] == [(P.COS, 384, 40_037, 256)]
    assert len({c["id"] for c in P.CASES}) == len(P.CASES) == 26
    assert {d for _, d, _ in SMALLEST} == {64, 100, 128, 192, 256, 384, 512, 768}


@pytest.mark.parametrize("case", P.CASES, ids=lambda c: c["id"])
def test_a_row_and_its_twin_never_share_a_place(case):
    metric, dims, n, nq = case["metric"], case["dims"], case["n"], case["nq"]
    h = n // 2
    tr = P.tile_rows(metric, dims)
    # the whole batches and the ragged last one (a different number of query groups, hence of workgroups per group)
    for q in {nq, n % nq or nq}:
        stride = P.stride_rows(metric, dims, n, q)
        assert h % stride != 0 and h % tr != 0, (case["id"], q, h, stride)
    assert n % nq != 0 and n % tr != 0, "the last batch and the last tile are ragged"
    pool = P.pool_first_row(metric, dims, n, nq)
    if case["route"] == P.POOL:
        per_group = P.workgroups_per_group(metric, dims, n, nq)
        assert per_group == 256 and P.n_tiles(metric, dims, n) // per_group == 24, "the smallest store with a pool"
        assert pool == 20 * 256 * tr and pool % tr == 0
        assert h < pool < n and 0 < pool - h < h, "twins on both sides of the pool's first tile: rows below pool - H have theirs in front of it"
    else:
        assert pool is None, case["id"]
    if case["route"] == P.GROUPS:
        assert P.query_groups(nq) == nq // 256 and P.workgroups_per_group(metric, dims, n, nq) == {512: 128, 768: 85, 1024: 64}[nq]
        assert P.query_groups(n % nq) == 1
    elif case["route"] in (P.POOL, P.FIXED, P.SPLIT, P.HANDLE, P.SLAB):
        assert P.is_rq(metric, dims) and P.query_groups(nq) == 1
    elif case["route"] == P.TILED:
        assert not P.is_rq(metric, dims) and dims % 64 == 0 and P.n_tiles(metric, dims, n) >= 512   # the one-pass plan's floor for this kernel
    if case["id"] == "clipped-cos384":
        assert P.workgroups_per_group(metric, dims, n, nq) == P.n_tiles(metric, dims, n) == 65 and n >= 64 * 64
    if case["id"] == "slab-below-floor":
        assert n < 64 * 64
    if case["route"] == P.HANDLE:
        block = -(-(-(-n // P.HANDLE_SHARDS)) // 64) * 64
        assert all((i // block) != ((i + h) // block) for i in (0, block - 1, block, h - 1)), "twins fall in different shards"


def test_eps_restated_and_the_cap_bound():
    # "0.0078" at the worst case for unit vectors; twice that under L2; the norms' product under dot
    assert 0.0078 < P.eps_worst(P.COS, 384, 1.0, 1.0) < 0.0079
    assert 0.0078 * 2.89 < P.eps_worst(P.DOT, 384, 1.7, 1.7) < 0.0080 * 2.89
    assert 0.0156 < P.eps_worst(P.L2, 384, 1.0, 1.0) < 0.0159
    # the bound against a Monte-Carlo count where it is loose enough to be seen: 2 000 unit vectors in R^8, t = 0.8
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2000, 8))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    s = x @ x.T
    np.fill_diagonal(s, 0.0)
    assert np.sum(s >= P.CAP_T) <= P.cap_bound(2000, 8)
    for metric, dims, n in P.stores():
        if (metric, dims, n) not in SMALLEST:
            assert P.cap_bound(n, dims) < P.CAP_SUM_MAX, (metric, dims, n)


@pytest.mark.parametrize("metric", [P.COS, P.DOT, P.L2])
def test_the_blocked_product_against_a_plain_one(metric):
    """stranger_best forms only the blocks on and above the diagonal: on a store of 301 rows with blocks of 64 it must give what the
    whole float64 score matrix gives; and the model's 32-bit bf16 rounding is helpers.bf16_rne."""
    import helpers
    n, dims = 301, 32
    rows = P.twin_store(metric, dims, n, seed=11)
    if metric != P.COS:
        rows = rows * np.linspace(0.8, 1.2, n, dtype=np.float32)[:, None]       # unequal norms: the row and column terms of L2 matter
    x = rows.astype(np.float64)
    s = x @ x.T
    if metric == P.COS:
        s /= np.outer(np.linalg.norm(x, axis=1), np.linalg.norm(x, axis=1))
    elif metric == P.DOT:
        s -= 1.0
    else:
        s = 2.0 * s - np.sum(x * x, axis=1)[:, None] - np.sum(x * x, axis=1)[None, :]
    p = P.partner(n)
    for i in range(n):
        s[i, i] = -np.inf
        if p[i] >= 0:
            s[i, p[i]] = -np.inf
    best = P.stranger_best(rows, metric, block=64)
    assert best.shape == (n,) and np.max(np.abs(best - np.max(s, axis=1))) < 1e-5
    v = np.concatenate([rows.ravel(), np.float32([0.0, -0.0, 1.0, 1.00390625, 1.01171875, -3.0e-39, 2.5e38])])
    assert np.array_equal(P._bf16(v).view(np.uint32), helpers.bf16_rne(v).view(np.uint32))


def test_drop_row_on_a_store_of_five():
    t3 = np.array([[0, 2, 4], [1, 3, 0], [2, 0, 3], [3, 1, 2], [4, 1, -1]])
    base = P.drop_row(t3, 99)
    assert base.tolist() == [[0, 2], [1, 3], [2, 0], [3, 1], [4, -1]]
    assert P.drop_row(t3, 2).tolist() == [[0, 4], [1, 3], [0, 3], [3, 1], [4, -1]]
    assert P.drop_row(t3, 1).tolist() == [[0, 2], [3, 0], [2, 0], [3, 2], [4, -1]]      # the lone row's stranger: its checked answer stays
    assert P.drop_row(t3, 4).tolist() == [[0, 2], [1, 3], [2, 0], [3, 1], [1, -1]]


@pytest.mark.parametrize("metric,dims,n", P.stores(), ids=lambda v: str(v))
def test_store_properties(metric, dims, n):
    rows = P.twin_store(metric, dims, n)
    h, p = n // 2, P.partner(n)
    assert rows.shape == (n, dims) and rows.dtype == np.float32
    # (a)
    cos = P.pair_cosines(rows)
    assert P.PAIR_COS_MIN <= cos.min() and cos.max() <= P.PAIR_COS_MAX, (cos.min(), cos.max())
    assert abs(float(np.median(cos)) - 1.0 / np.sqrt(1.0 + P.SIGMA ** 2)) < 0.005
    norms = np.linalg.norm(rows.astype(np.float64), axis=1)
    want = P.DOT_SCALE if metric == P.DOT else 1.0
    assert np.max(np.abs(norms - want)) < 1e-6, "one common norm: dot = s^2 cos and |a - b|^2 = 2 s^2 (1 - cos) order the rows as the cosine does"
    ids, scores = P.expected(rows, metric)
    paired = p >= 0
    assert np.array_equal(ids[:, 0], np.arange(n)) and np.array_equal(ids[paired, 1], p[paired]) and np.all(ids[~paired, 1] == -1)
    assert np.all(scores[paired, 0] > scores[paired, 1]) and np.all(np.isnan(scores[~paired, 1])) and int(np.sum(~paired)) == n % 2
    unit = P.DISTANCE_UNIT[metric]
    self_score = {P.COS: 1.0, P.DOT: want * want - 1.0, P.L2: 0.0}[metric]
    assert np.max(np.abs(scores[:, 0] - self_score)) < 1e-6
    gap = (scores[paired, 0] - scores[paired, 1]) / unit
    assert np.max(np.abs(gap - (1.0 - cos[np.arange(n)[paired] % h]))) < 1e-6      # rank 2 is the pair's cosine in the metric's units
    # (b)
    if (metric, dims, n) in SMALLEST:
        t3, best = P.top3(rows, metric)                             # asserts self > twin > best stranger for every query
        print(f"\n[{P.METRIC_NAME[metric]} {dims} x {n}] best stranger {float(np.max((best - self_score) / unit + 1.0)):.3f} (cosine), "
              f"pairs {cos.min():.3f} .. {cos.max():.3f}")
    else:
        assert P.cap_bound(n, dims) < P.CAP_SUM_MAX and cos.min() > P.CAP_T
        t3 = P.strangers_behind(ids)                                # by the bound every stranger ranks behind the twin
    # (c)
    sample = P.margin_sample(n)
    assert len(sample) >= P.MARGIN_SAMPLE
    margins = P.certificate_margins(rows, metric, sample) / unit
    print(f"[{P.METRIC_NAME[metric]} {dims} x {n}] certificate margin {margins.min():.3f} .. {margins.max():.3f}")
    assert margins.min() > P.MARGIN_MIN, margins.min()
    # (d)
    checked = P.drop_row(t3, -7)
    assert np.array_equal(checked, ids)
    seen = np.bincount(checked[checked >= 0], minlength=n)
    assert np.all(seen[paired] == 2) and np.all(seen[~paired] == 1), "every row position is required at rank 1 and, if it has a twin, at rank 2"
    rng = np.random.default_rng(n + dims)
    for r in [0, h - 1, h, 2 * h - 1, n - 1] + rng.integers(0, n, 27).tolist():
        changed = np.flatnonzero(np.any(P.drop_row(t3, r) != checked, axis=1))
        assert changed.tolist() == sorted({r, int(p[r])} - {-1}), (r, changed)
