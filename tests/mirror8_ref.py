"""The 8-bit code mirror restated on the CPU (numpy): the quantiser, the per-row error, the lower-bound key, the slack and the
certificate of DESIGN 4.1 "Eight bits per element", plus the stores and queries the two mirror8 test files share. No engine code runs
here: test_mirror8_cpu.py proves properties of these inputs, test_mirror8_gpu.py asserts what follows from them on the device."""
import numpy as np

import oracle

KP = 64            # candidates kept (MIRROR_KP)
MAX_K = 16         # largest k the code mirror answers (MIRROR8_MAX_K)
U = 5.97e-8        # 2^-24, rounded up as the kernels write it
TINY = 2.0 ** -149  # the smallest f32: what one rounding costs in the subnormal range

GAUSSIAN_SHAPES = [(20005, 384), (5003, 768)]     # neither is a multiple of the rows per chunk (32 at 384-d, 16 at 768-d)
N_QUERIES = 8


def corpus_for(metric, n, dims, seed=0):
    """Unit Gaussian rows; dot: rows of different norms (test_mirror_scan_gpu.py's construction)."""
    x = oracle.gaussian_unit_rows(seed, n, dims)
    if metric == 1:
        x = x * np.random.default_rng(seed + 7).uniform(0.5, 2.0, size=(n, 1)).astype(np.float32)
    return np.ascontiguousarray(x, dtype=np.float32)


def queries_for(dims, n=N_QUERIES):
    return oracle.gaussian_unit_queries(n, dims)


def duplicate_store(q, n=10000, dims=384, dups=2048):
    x = corpus_for(0, n, dims, seed=41).copy()
    x[100:100 + dups] = q
    return x


def clustered_store(q, n=10000, dims=384):
    rng = np.random.default_rng(45)
    centre = q / np.linalg.norm(q)
    return (centre[None, :] + 1e-3 * rng.standard_normal((n, dims))).astype(np.float32)


def outlier_store(n=10000, dims=384, row=1234):
    """One row with a single huge element (0.7 of the row's norm, 30 times its neighbours'): the row's scale follows that element,
    every other element of it rounds coarsely, and its err is several times the store's typical one — for that row only. The rest of
    the row points at the mean of the shared queries (cosine ~0.25 to each), so it is near the top of every answer: its coarse key must
    not cost it its place."""
    x = corpus_for(0, n, dims, seed=47).copy()
    v = np.sum(queries_for(dims).astype(np.float64), axis=0)
    x[row] = (v / np.linalg.norm(v)).astype(np.float32)
    x[row, 5] = 1.0
    return x


OUTLIER_ROW = 1234


def zero_row_store(n=10000, dims=384):
    x = corpus_for(0, n, dims, seed=41).copy()
    x[20:5000] = 0.0
    return x


def normalise(x, metric):
    """x^: what the codes approximate. Cosine: the row over its f32 norm, rows of norm <= 1e-6 (or NaN) zero; dot: the row."""
    x = np.asarray(x, dtype=np.float32)
    if metric != 0:
        return x
    with np.errstate(all="ignore"):
        n = np.sqrt(np.sum(x.astype(np.float32) ** 2, axis=1, dtype=np.float32))
        out = (x * (np.float32(1.0) / n)[:, None]).astype(np.float32)
    out[~(n > np.float32(1e-6))] = 0.0
    return out


def quantise(xhat):
    """-> codes (int16 in [-127, 127]), scale (f32), err (f32, rounded up; +inf for a row that cannot be coded)."""
    xhat = np.asarray(xhat, dtype=np.float32)
    dims = xhat.shape[1]
    with np.errstate(all="ignore"):
        bad = ~np.all(np.isfinite(xhat), axis=1)
        amax = np.max(np.abs(np.where(np.isfinite(xhat), xhat, 0.0)), axis=1).astype(np.float32)
        scale = (amax / np.float32(127.0)).astype(np.float32)
        t = np.where(scale[:, None] > 0, xhat / np.where(scale > 0, scale, 1)[:, None], 0.0)
        t = np.where(np.isnan(t), 0.0, t)
        codes = np.rint(np.clip(t, -127.0, 127.0)).astype(np.int16)
        diff = scale.astype(np.float64)[:, None] * codes - xhat.astype(np.float64)
        err = np.sqrt(np.sum(diff * diff, axis=1))
        err64 = err * (1.0 + dims * 2.0 ** -23)
        err = err64.astype(np.float32)
        err = np.where(err < err64, np.nextafter(err, np.float32(np.inf)), err).astype(np.float32)     # rounded up, never down
        err = np.where(err == 0, np.float32(TINY), err)              # (the kernel's err is never 0: a zero row has the smallest f32)
    bad |= ~np.isfinite(scale) | ~np.isfinite(err)
    scale = np.where(bad, np.float32(0.0), scale).astype(np.float32)
    err = np.where(bad, np.float32(np.inf), err).astype(np.float32)
    return codes, scale, err


def approx_dots(q, codes, scale):
    """scale_r * sum_i q_i code_ri, in f64."""
    return scale.astype(np.float64) * (codes.astype(np.float64) @ np.asarray(q, dtype=np.float64))


def lower_bounds(q, codes, scale, err, metric):
    qn = float(np.linalg.norm(np.asarray(q, dtype=np.float64)))
    s = approx_dots(q, codes, scale)
    with np.errstate(all="ignore"):
        lb = 1.0 - s / qn - err if metric == 0 else 1.0 - s - qn * err.astype(np.float64)
    return np.where(np.isnan(lb), -np.inf, lb)


def slack(dims, metric, q_norm, max_norm):
    """mirror8_slack (mirror8_scan.hip): f32 accumulation of the biased sum, sums and normalisations, the key's own roundings."""
    qn = 1.0 + 1e-6 if metric == 0 else float(q_norm)
    vn = 1.0 + 1e-6 if metric == 0 else float(max_norm)
    both = (8192.0 * U * np.sqrt(dims) / 127.0 + 3.0 * dims * U) * qn * vn * 1.001
    return both + (3e-6 if metric == 0 else 3e-6 * (1.0 + qn * vn))


def exact_distances(x, q, metric):
    x64, q64 = np.asarray(x, dtype=np.float64), np.asarray(q, dtype=np.float64)
    with np.errstate(all="ignore"):
        dot = x64 @ q64
        if metric != 0:
            d = 1.0 - dot
        else:
            n = np.linalg.norm(x64, axis=1)
            qn = np.linalg.norm(q64)
            d = 1.0 - np.where((n > 1e-6) & (qn > 1e-6), dot / (n * qn), 0.0)
    return np.where(np.isnan(d), np.inf, d)


class Coded:
    """A store with its code mirror, built once and shared."""

    def __init__(self, x, metric):
        self.x, self.metric = x, metric
        self.xhat = normalise(x, metric)
        self.codes, self.scale, self.err = quantise(self.xhat)
        with np.errstate(all="ignore"):
            n = np.linalg.norm(x.astype(np.float64), axis=1)
        self.max_norm = float(np.max(n[np.isfinite(n)])) if np.any(np.isfinite(n)) else 0.0

    def margin(self, q, k):
        """lb_KP - slack - d_k: the certificate holds iff this is > 0 and finite (NaN query: never)."""
        q = np.asarray(q, dtype=np.float32)
        if not np.all(np.isfinite(q)) or len(self.x) < KP:
            return -np.inf
        lb = lower_bounds(q, self.codes, self.scale, self.err, self.metric)
        cand = np.argsort(lb, kind="stable")[:KP]
        lb_kp = lb[cand[-1]]
        d = np.sort(exact_distances(self.x[cand], q, self.metric))
        qn = float(np.linalg.norm(q.astype(np.float64)))
        if not np.isfinite(lb_kp) or not np.isfinite(d[k - 1]):
            return -np.inf
        return lb_kp - slack(self.x.shape[1], self.metric, qn, self.max_norm) - d[k - 1]


class MaskedModel:
    """The certificate of a masked pass (the predicate tickets'): lower bounds and exact distances of every (row, query) of one
    store, and the slack per query."""

    def __init__(self, metric, rows, qs):
        coded = Coded(rows, metric)
        self.lb = np.stack([lower_bounds(q, coded.codes, coded.scale, coded.err, metric) for q in qs], axis=1)
        self.exact = np.stack([exact_distances(rows, q, metric) for q in qs], axis=1)
        self.slack = np.array([slack(rows.shape[1], metric, float(np.linalg.norm(q.astype(np.float64))), coded.max_norm) for q in qs])

    def margin(self, mask, q, k):
        """lb_64 - slack - d_k: the 64 best lower bounds among the passing rows, the exact k-th distance among those 64 rows."""
        rows = np.flatnonzero(mask)
        if len(rows) <= KP:
            return -np.inf
        lb = self.lb[rows, q]
        cand = np.argsort(lb, kind="stable")[:KP]
        d = np.sort(self.exact[rows[cand], q])
        return float(lb[cand[-1]] - self.slack[q] - d[k - 1])


# ---------------------------------------------------------------------------
# The device's code mirror held to float64 (test_mirror8_edges_gpu.py reads it through mirror8Snapshot; test_mirror8_cpu.py proves
# that an IEEE f32 quantiser passes every check below and that a halved err, a swapped byte pair or a wrong scale does not).

F32_MAX = float(np.finfo(np.float32).max)


def to_bytes(codes):
    """codes in [-127, 127] -> the biased bytes as stored."""
    return (np.asarray(codes, dtype=np.int16) + 128).astype(np.uint8)


def expected_max_norm(x):
    """The max-norm word of a store: the largest row norm, NaN norms left out; +inf when a row's sum of squares leaves the f32 range
    (or holds an inf). None: a row sits too close to the f32 limit for float64 to say which."""
    x64 = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        m = np.sum(x64 * x64, axis=1)
    m = m[~np.isnan(m)]
    if m.size == 0:
        return 0.0
    if np.any((m > F32_MAX * 0.99) & (m < F32_MAX * 1.01)):
        return None
    return float(np.inf) if np.any(m >= F32_MAX * 1.01) else float(np.sqrt(np.max(m)))


def check_max_norm(x, word, ctx=""):
    """The word equals the largest finite row norm within (D + 4) 2^-24 relative; +inf when a row's norm overflows."""
    want = expected_max_norm(x)
    assert want is not None, f"{ctx}: a row norm at the f32 limit: the store does not decide the word"
    if np.isinf(want):
        assert word == np.inf, f"{ctx}: max-norm word {word}, a row norm overflows"
    else:
        assert abs(word - want) <= (np.shape(x)[1] + 4) * 2.0 ** -24 * want, f"{ctx}: max-norm word {word} != {want}"


def check_rows(x, metric, codes_u8, scale, err, ctx=""):
    """Every row of a code mirror (biased bytes, scale, err as the device holds them) against the f64 rows x they were made from.
    x^ = the f64 row, for cosine over its f64 norm; rho = (D + 4) 2^-24 ||x^|| (cosine: the f32 norm and scaling the kernel
    normalises with), 0 for dot (the kernel codes the stored floats themselves). Per row:
      bytes      in [1, 255];
      codes      |scale (byte - 128) - x^_i| <= scale (0.5 + t_i) + rho, t_i = max(2^-20, (|code_i| + 1) 2^-24): the code is rint of the
                 f32 quotient x^_i / scale, which sits within 2^-24 |x^_i / scale| of the exact one (2^-18 at |code| >= 64: a flat 2^-20
                 is not what correctly rounded f32 division gives, test_mirror8_cpu.py shows an element beyond it);
      scale      |scale - max|x^| / 127| <= 2^-22 scale + rho / 127 + 2^-149 (the last: a quotient in the subnormal range is rounded to
                 a multiple of 2^-149, not to 2^-24 relative);
      soundness  err >= ||scale (byte - 128) - x^||_2 - rho;
      tightness  err <= that norm (1 + D 2^-22) + rho + 2^-149;
      rows that cannot be coded (dot: an inf or NaN element; cosine: an inf element and no NaN)  err == +inf, scale == 0;
      cosine rows whose norm is NaN or <= 1e-6  scale == 0, all bytes 128, err <= 1e-44.
    Returns the number of rows in each class."""
    x64 = np.asarray(x, dtype=np.float64)
    n, dims = x64.shape
    b = np.asarray(codes_u8)
    scale64, err64 = np.asarray(scale, dtype=np.float64), np.asarray(err, dtype=np.float64)
    assert b.shape == (n, dims) and b.dtype == np.uint8 and scale64.shape == (n,) and err64.shape == (n,), f"{ctx}: shapes"
    assert b.min() >= 1, f"{ctx}: byte 0 at row {int(np.argmin(b.min(axis=1)))}"
    with np.errstate(all="ignore"):
        finite = np.all(np.isfinite(x64), axis=1)
        norm = np.sqrt(np.sum(x64 * x64, axis=1))
        if metric == 0:
            zero = np.isnan(norm) | (norm <= 1e-6)
            lost = ~zero & np.isinf(norm)
            ok = ~zero & ~lost
            assert not np.any(ok & ((np.abs(norm - 1e-6) < 1e-9) | (norm > 1e18))), f"{ctx}: a cosine row at the zero-row rule or beyond the f32 norm"
            xhat = np.where(ok[:, None], x64 / np.where(ok, norm, 1.0)[:, None], 0.0)
            rho = (dims + 4) * 2.0 ** -24
        else:
            zero = np.zeros(n, dtype=bool)
            lost = ~finite
            ok = finite
            xhat = np.where(ok[:, None], x64, 0.0)
            rho = 0.0
    assert np.all(np.isposinf(err64[lost])) and np.all(scale64[lost] == 0), \
        f"{ctx}: rows that cannot be coded {np.flatnonzero(lost)[:5]}: err {err64[lost][:5]}, scale {scale64[lost][:5]}"
    assert np.all(scale64[zero] == 0) and np.all(b[zero] == 128) and np.all(err64[zero] <= 1e-44) and np.all(err64[zero] >= 0), \
        f"{ctx}: zero rows {np.flatnonzero(zero)[:5]}"
    rows = np.flatnonzero(ok)
    c = b[rows].astype(np.float64) - 128.0
    s, e, xh = scale64[rows], err64[rows], xhat[rows]
    assert np.all(np.isfinite(s)) and np.all(s >= 0) and np.all(np.isfinite(e)) and np.all(e >= 0), f"{ctx}: scale / err not finite on codable rows {rows[~(np.isfinite(s) & np.isfinite(e))][:5]}"
    diff = s[:, None] * c - xh
    tol = s[:, None] * (0.5 + np.maximum(2.0 ** -20, (np.abs(c) + 1.0) * 2.0 ** -24)) + rho
    bad = np.abs(diff) > tol
    assert not bad.any(), f"{ctx}: {int(bad.sum())} codes are not the rounded ones, first at row {rows[np.argwhere(bad)[0][0]]} element {np.argwhere(bad)[0][1]}"
    want = np.max(np.abs(xh), axis=1) / 127.0
    bad = np.abs(s - want) > 2.0 ** -22 * s + rho / 127.0 + TINY
    assert not bad.any(), f"{ctx}: scale of rows {rows[bad][:5]}: {s[bad][:5]} != {want[bad][:5]}"
    moved = np.sqrt(np.sum(diff * diff, axis=1))
    bad = e < moved - rho
    assert not bad.any(), f"{ctx}: err is no bound on rows {rows[bad][:5]}: err {e[bad][:5]} < {moved[bad][:5]}"
    bad = e > moved * (1.0 + dims * 2.0 ** -22) + rho + TINY
    assert not bad.any(), f"{ctx}: err is loose on rows {rows[bad][:5]}: err {e[bad][:5]} > {moved[bad][:5]}"
    return {"coded": int(ok.sum()), "zero": int(zero.sum()), "lost": int(lost.sum())}


def non_finite_store(metric, dims=384):
    """test_mirror8_gpu.py's inf / NaN / zero-block store."""
    odd = corpus_for(metric, 5003, dims, seed=43).copy()
    odd[7, 3] = np.inf
    odd[9, 11] = np.nan
    odd[4000:4100] = 0.0
    return odd


EXTREME_SUBNORMAL, EXTREME_HUGE, EXTREME_HUGER, EXTREME_FLAT = slice(10, 40), slice(50, 80), slice(90, 96), 100


def extreme_dot_store(n=300, dims=384):
    """A dot store whose rows leave the range f32 squares live in: rows [10, 40) have subnormal elements (Gaussian times 1e-41 ..
    1e-39: the squares of their rounding differences are 0 in f32), rows [50, 80) lie near 1e19 (the squares of the elements
    overflow, so the row norm is +inf), rows [90, 96) near 1e21 (there the squares of the rounding differences overflow too: the
    row's err itself, ~5e19, is an ordinary f32), and row 100 has every element +-0.37, so all its codes are +-127."""
    rng = np.random.default_rng(53)
    x = corpus_for(1, n, dims, seed=51).astype(np.float64)
    g = rng.standard_normal((n, dims))
    for rows, lo, hi in ((EXTREME_SUBNORMAL, 1e-41, 1e-39), (EXTREME_HUGE, 0.5e19, 2e19), (EXTREME_HUGER, 0.5e21, 2e21)):
        k = rows.stop - rows.start
        x[rows] = g[rows] * np.geomspace(lo, hi, k)[:, None]
    x[EXTREME_FLAT] = np.where(g[EXTREME_FLAT] > 0, 0.37, -0.37)
    return np.ascontiguousarray(x, dtype=np.float32)


# ---------------------------------------------------------------------------
# A row whose quantisation error is aligned with the query (test (c) of test_mirror8_edges_gpu.py).

ALIGNED_ROW, ALIGNED_N, ALIGNED_NEIGHBOURS = 1234, 4000, 300
ALIGNED_NEAR, ALIGNED_FAR = 0.004, 0.02


def aligned_row(dims):
    """A unit row with one element of 127 code units and every other at +-1.49 units: each of those rounds to +-1 and loses a third
    of itself, all in the row's own direction. Its approximate self-distance is ~0.016 (384-d) while its err is ~0.074."""
    rng = np.random.default_rng(61)
    a = 1.49 * np.where(rng.random(dims) < 0.5, -1.0, 1.0)
    a[7] = 127.0
    return (a / np.linalg.norm(a)).astype(np.float32)


def aligned_store(dims, metric=0, appended=False):
    """(rows, A, A's row): Gaussian rows, ALIGNED_NEIGHBOURS honest neighbours of A at cosine distances graded from 0.004 to 0.02
    (they share A's large element, hence its scale, but their small elements round both ways), and A itself at row ALIGNED_ROW —
    or, `appended`, left out of the rows (a Gaussian row takes its place) for the caller to add after the mirror is built. For dot
    every row is scaled to norm 3; the query is then 2 A / ||A||."""
    rng = np.random.default_rng(67)
    x = corpus_for(0, ALIGNED_N, dims, seed=59).astype(np.float64)
    a = aligned_row(dims).astype(np.float64)
    a /= np.linalg.norm(a)
    cos = 1.0 - np.linspace(ALIGNED_NEAR, ALIGNED_FAR, ALIGNED_NEIGHBOURS)
    where = rng.permutation(np.delete(np.arange(ALIGNED_N), ALIGNED_ROW))[:ALIGNED_NEIGHBOURS]
    x[where] = cos[:, None] * a[None, :] + np.sqrt(1.0 - cos * cos)[:, None] * _orthogonal_units(rng, a, ALIGNED_NEIGHBOURS)
    if not appended:
        x[ALIGNED_ROW] = a
    if metric == 1:
        x *= 3.0
        a = a * 3.0
    return np.ascontiguousarray(x, dtype=np.float32), a.astype(np.float32), ALIGNED_ROW


def aligned_query(a, metric):
    a64 = a.astype(np.float64)
    return (a64 / np.linalg.norm(a64) * (2.0 if metric == 1 else 1.0)).astype(np.float32)


def _orthogonal_units(rng, qhat, count):
    u = rng.standard_normal((count, qhat.size))
    u -= (u @ qhat)[:, None] * qhat[None, :]
    return u / np.linalg.norm(u, axis=1)[:, None]


# ---------------------------------------------------------------------------
# The certificate decision on a ladder (test (d)).

LADDER_N, LADDER_RUNGS, LADDER_QUERIES, LADDER_FIRST = 6000, 200, 8, 0.05


def ladder_store(dims, metric):
    """(rows, queries): LADDER_N Gaussian rows (dot: of norms 0.5 .. 1, so that the unit rungs are the longest rows) and LADDER_RUNGS
    unit rungs at controlled cosine distances from the first query. The first 16 stand three slacks apart from LADDER_FIRST on, so
    margin(k) = lb_KP - slack - d_k moves by three slacks per k and at most one k can fall inside |margin| <= slack. The others start
    three slacks above the sixteenth and are spaced so that the 48th of them — the 64th key of the store — has its key (~err below
    its distance) halfway between the eighth and the ninth: k <= 8 certify, k >= 9 do not, give or take what
    each of the LADDER_QUERIES queries (the first and seven within 2e-3 of it) sees differently."""
    rng = np.random.default_rng(71 + dims + metric)
    x = corpus_for(0, LADDER_N + LADDER_RUNGS, dims, seed=73).astype(np.float64)
    if metric == 1:
        x *= rng.uniform(0.5, 1.0, size=(len(x), 1))
    q = queries_for(dims, 1)[0].astype(np.float64)
    q /= np.linalg.norm(q)
    sl = slack(dims, metric, 1.0, 1.0)
    units = _orthogonal_units(rng, q, LADDER_RUNGS)

    def rungs(dist):
        c = 1.0 - dist
        return (c[:, None] * q[None, :] + np.sqrt(1.0 - c * c)[:, None] * units[:len(dist)]).astype(np.float32)

    first = LADDER_FIRST + 3.0 * sl * np.arange(16)
    err = float(np.median(quantise(rungs(first))[2]))
    rest0, rest47 = first[-1] + 3.0 * sl, first[0] + 23.5 * sl + err        # key of the 48th: rest47 - err = (first[7] + first[8]) / 2 + sl
    assert rest47 > rest0
    rest = rest0 + (rest47 - rest0) / 47.0 * np.arange(LADDER_RUNGS - 16)
    for _ in range(3):      # a rung's key is not exactly err below its distance: move the upper rungs until margin(8) = +1.5 slacks for the first query
        r = rungs(np.concatenate([first, rest]))
        lb = np.sort(lower_bounds(q.astype(np.float32), *quantise(normalise(r, metric)), metric))
        rest = rest + (first[7] + 2.5 * sl - lb[KP - 1])
    assert rest[0] > first[-1] + sl
    x = x.astype(np.float32)
    x[LADDER_N:] = rungs(np.concatenate([first, rest]))
    queries = [q] + [q + 2e-3 * w for w in _orthogonal_units(rng, q, LADDER_QUERIES - 1)]
    queries = np.stack([v / np.linalg.norm(v) for v in queries]).astype(np.float32)
    return np.ascontiguousarray(x), queries


def ladder_expectations(coded, queries):
    """[(query index, k, margin, slack)] for k = 1 .. MAX_K."""
    out = []
    for i, q in enumerate(queries):
        qn = float(np.linalg.norm(q.astype(np.float64)))
        sl = slack(coded.x.shape[1], coded.metric, qn, coded.max_norm)
        out += [(i, k, coded.margin(q, k), sl) for k in range(1, MAX_K + 1)]
    return out


# ---------------------------------------------------------------------------
# Row-count edges of the scan (test (e)).

def scan_edge_counts(dims):
    rpc = 64 // (dims // 24) * 8          # rows per wave iteration: 32 at 384-d, 16 at 768-d
    return sorted({1, 63, 64, 65, 2 * rpc - 1, 2 * rpc, 2 * rpc + 1})
