"""The query side of the 8-bit pass on the matrix pipe, restated on the CPU (numpy): the three-digit quantiser of the query, the
integer sum, the key, and the data that test_mirror8_planes_cpu.py and test_mirror8_mfma_gpu.py share (DESIGN 4.1 "Eight bits per
element"). The row side — codes, scale, err, slack — is mirror8_ref.py's. No engine code runs here."""
import functools

import numpy as np

import mirror8_ref as R8
import oracle

M = 63 * 16384 + 63 * 128 + 63      # the largest |m_i|: 1 040 319
U = 2.0 ** -24

# the stores and queries of test_mirror_pass_forms_gpu.py (restated: a test module is not imported by another)
N, N_QUERIES, STORE_SEED, QUERY_SEED = 1003, 8, 20261019, 11
SMALL_N = 15                         # less than one 16-row tile
CASES = [(m, d) for m in (0, 1) for d in (384, 768)]
CASE_IDS = [f"{'cosine' if m == 0 else 'dot'}-{d}" for m, d in CASES]


@functools.lru_cache(maxsize=None)
def store_rows(metric, dims):
    x = oracle.gaussian_unit_rows(0, N, dims, seed=STORE_SEED)
    if metric == 1:                  # dot: rows of norms 0.5 .. 2
        x = x * np.random.default_rng(STORE_SEED + 7).uniform(0.5, 2.0, size=(N, 1)).astype(np.float32)
    return np.ascontiguousarray(x, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def queries(dims):
    return oracle.gaussian_unit_queries(N_QUERIES, dims, seed=QUERY_SEED)


@functools.lru_cache(maxsize=None)
def coded(metric, dims):
    return R8.Coded(store_rows(metric, dims), metric)


def mixed_k(i):
    """The k of query i in the end-to-end test, besides 1 and 16: 4, 9, 14, 3, 8, 13, 2, 7."""
    return 1 + (5 * i + 3) % R8.MAX_K


# ---------------------------------------------------------------------------
# The quantiser: every step in IEEE f32, as the kernel's prologue does it.

def delta_of(q):
    """max|q| / M in f32; NaN for a query with a non-finite element (its keys can never certify); 0 below the normal range."""
    q = np.asarray(q, dtype=np.float32)
    if not np.all(np.isfinite(q)):
        return np.float32(np.nan)
    delta = np.float32(np.max(np.abs(q))) / np.float32(M)
    return delta if delta >= np.finfo(np.float32).tiny else np.float32(0.0)     # (a subnormal delta has no f32 reciprocal)


def quantise(q):
    """-> (m int64 [D], delta f32): m_i = rint(q_i * (1 / delta)) clamped to +-M, reciprocal and product each rounded to f32 as the
    kernel does; delta 0 or NaN: no digits."""
    q = np.asarray(q, dtype=np.float32)
    delta = delta_of(q)
    if not delta > 0:
        return np.zeros(q.shape, dtype=np.int64), delta
    with np.errstate(all="ignore"):
        t = (q * (np.float32(1.0) / delta)).astype(np.float32)
    t = np.where(np.isnan(t), np.float32(0), t)
    return np.rint(np.clip(t, -float(M), float(M))).astype(np.int64), delta


def digits(m):
    """m = 16384 a + 128 b + c, balanced: every digit in [-64, 63]."""
    m = np.asarray(m, dtype=np.int64)
    c = ((m + 64) & 127) - 64
    m1 = (m - c) >> 7
    b = ((m1 + 64) & 127) - 64
    a = (m1 - b) >> 7
    return a, b, c


def integer_sums(codes, m):
    """S_r = sum_i m_i code_ri, exact."""
    return np.asarray(codes, dtype=np.int64) @ np.asarray(m, dtype=np.int64)


def keys64(q, codes, scale, err, metric):
    """The key of every row in f64 from the exact integer sum: the f64 model of the quantised form. NaN -> -inf."""
    m, delta = quantise(q)
    qn = float(np.linalg.norm(np.asarray(q, dtype=np.float64)))
    with np.errstate(all="ignore"):
        s = float(delta) * scale.astype(np.float64) * integer_sums(codes, m).astype(np.float64)
        if metric == 0:
            lb = 1.0 - s * (1.0 / qn if qn > 1e-6 else 0.0) - err.astype(np.float64)
        else:
            lb = 1.0 - s - qn * err.astype(np.float64)
    return np.where(np.isnan(lb), -np.inf, lb)


def term_a(dims, q_norm, max_norm):
    """Term (a) of the slack (mirror8_ref.slack's first summand, with its norms)."""
    return 8192.0 * R8.U * np.sqrt(dims) / 127.0 * q_norm * max_norm


def margin(cd, q, k):
    """R8.Coded.margin with the keys of the quantised form: lb_KP - slack - d_k."""
    q = np.asarray(q, dtype=np.float32)
    if not np.all(np.isfinite(q)) or len(cd.x) < R8.KP:
        return -np.inf
    lb = keys64(q, cd.codes, cd.scale, cd.err, cd.metric)
    cand = np.argsort(lb, kind="stable")[:R8.KP]
    d = np.sort(R8.exact_distances(cd.x[cand], q, cd.metric))
    if not np.isfinite(lb[cand[-1]]) or not np.isfinite(d[k - 1]):
        return -np.inf
    qn = float(np.linalg.norm(q.astype(np.float64)))
    return lb[cand[-1]] - R8.slack(cd.x.shape[1], cd.metric, qn, cd.max_norm) - d[k - 1]


def adversarial_queries(dims):
    """{name: query}: what a quantiser scaled by max|q| can get wrong."""
    rng = np.random.default_rng(83 + dims)
    g = rng.standard_normal(dims).astype(np.float32)
    out = {}
    v = g.copy(); v[dims // 3] = 50.0 * np.max(np.abs(g)); out["one element 50 x the rest"] = v
    out["all elements equal"] = np.full(dims, 0.37, dtype=np.float32)
    out["magnitude 1e-30"] = (g * np.float32(1e-30)).astype(np.float32)
    out["magnitude 1e30"] = (g * np.float32(1e30)).astype(np.float32)
    out["all zero"] = np.zeros(dims, dtype=np.float32)
    v = g.copy(); v[::3] = 0.0; v[1::6] = -0.0; out["zeros and -0.0"] = v
    v = g.copy(); v[5] = np.nan; out["a NaN element"] = v
    v = g.copy(); v[7] = np.inf; out["an inf element"] = v
    return out


NON_FINITE = ("a NaN element", "an inf element")


# ---------------------------------------------------------------------------
# Exact data for the layout check: integer rows and an integer query whose sums fit 24 bits.

def layout_store(n, dims):
    """Integer rows, each with one 127 (so a dot row's scale is exactly 1 and its codes are the row) at a place that moves with the
    row, and a few small values at places and with signs that differ from row to row: no two rows are equal, and no permutation of
    the elements leaves every row's sum with the query below unchanged."""
    x = np.zeros((n, dims), dtype=np.float32)
    for r in range(n):
        big = (7 * r + 3) % dims
        if big == 0:
            big = 1
        x[r, big] = 127.0
        for j in range(1, 6):
            p = (big + 53 * j + r // dims + 11 * (r % 5)) % dims
            if p != big:
                x[r, p] = float((j + r) % 7 - 3)
        x[r, 0] = float(r % 3)          # the query's largest element: digit a = 63
    return x


def layout_query(dims):
    """Distinct integers, no symmetry over the elements: element 0 is M (so delta is exactly 1 and m = q), the others alternate in
    sign and grow by 37 per element, which fills digits b and c everywhere and digit a from element 222 on."""
    i = np.arange(dims, dtype=np.int64)
    m = (37 * i + 1) * np.where(i % 3 == 1, -1, 1)
    m[0] = M
    return m.astype(np.float32)
