"""The 8-bit code mirror restated on the CPU (numpy): the quantiser, the per-row error, the lower-bound key, the slack and the
certificate of DESIGN 4.1 "Eight bits per element", plus the stores and queries the two mirror8 test files share. No engine code runs
here: test_mirror8_cpu.py proves properties of these inputs, test_mirror8_gpu.py asserts what follows from them on the device."""
import numpy as np

import oracle

KP = 64            # candidates kept (MIRROR_KP)
MAX_K = 16         # largest k the code mirror answers (MIRROR8_MAX_K)
U = 5.97e-8        # 2^-24, rounded up as the kernels write it

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
        err = (err * (1.0 + dims * 2.0 ** -23)).astype(np.float32)
        err = np.nextafter(err, np.float32(np.inf))
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
