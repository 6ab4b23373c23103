"""The stores, masks and the float64 model behind tests/test_predicate_mirror_cpu.py and tests/test_predicate_mirror_gpu.py.

The route under test ("predicate_mirror"): a predicate query that the route rule sends to the masked scan streams the
bf16 mirror under the row bitmap, keeps the 64 best APPROXIMATE distances among the passing rows, re-scores those rows in f32 and
returns the k best only when
    a_64 - eps > d_k        (a_64: the 64th approximate distance among the passing rows, d_k: the exact k-th, eps: the finish kernel's bound)
Otherwise the masked f32 scan answers. The model computes the three terms in float64 from the same inputs: the GPU test asserts
zero fallbacks only on (store, mask, query, k) for which the CPU test has shown the margin a_64 - eps - d_k to be well above the
f32 summation error of the kernels, and asserts a fallback for every query only where the model's margin is negative."""
import functools

import numpy as np

import oracle
from helpers import bf16_rne

COS, DOT = 0, 1
MIRROR_KP = 64                   # candidates the finish kernel re-scores
MIRROR_MAX_K = 32                # largest top_k the mirror answers
MIRROR_CHUNK = {384: 16, 768: 8} # rows per chunk of the mirror form (mirror_scan_masked_kernel)
F32_CHUNK = {384: 8, 768: 2}     # rows per chunk of the masked f32 scan
STORE_SEED, QUERY_SEED, N_QUERIES = 20260220, 7, 16
KS = (1, 10, 32)
# Both sides of the certificate are f32 sums of D products of magnitudes <= 1 * max||v||: each within 3 D 2^-24 (1.4e-4 at 768-d) of
# its f64 value for unit rows, twice that for the dot stores' norms <= 2. The floor leaves the sum of both sides' errors (5.5e-4 in
# the worst of these stores) below it.
MARGIN_FLOOR = 1e-3

# name -> (metric, rows, dims)
STORES = {"cos384": (COS, 20_005, 384), "cos768": (COS, 3_001, 768), "dot384": (DOT, 20_005, 384), "dot768": (DOT, 3_001, 768)}
# the masks on which the GPU test asserts zero fallbacks (every k of KS, every query it sends)
TAKEN_MASKS = ("r15", "half", "range", "one_per_chunk", "tail_plus_65", "m65")
NOT_TAKEN_MASKS = ("m64", "m0")
MASK_BIT = {name: 1 << (8 + i) for i, name in enumerate(("r15", "half", "one_per_chunk", "tail_plus_65", "m65", "m64", "m0"))}


@functools.lru_cache(maxsize=None)
def store_rows(name):
    metric, n, dims = STORES[name]
    x = oracle.gaussian_unit_rows(0, n, dims, seed=STORE_SEED)
    if metric == DOT:                # rows of norms 0.5 .. 2
        x = x * np.random.default_rng(STORE_SEED + 7).uniform(0.5, 2.0, size=(n, 1)).astype(np.float32)
    x = np.ascontiguousarray(x, dtype=np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def queries(dims):
    q = oracle.gaussian_unit_queries(N_QUERIES, dims, seed=QUERY_SEED)
    q.setflags(write=False)
    return q


def range_bounds(n):
    """The contiguous range [lo, hi) of the "range" mask: 12 000 of 20 005 rows (in proportion for a smaller store), both ends inside a chunk."""
    lo = n // 5 + 3
    return lo, lo + (12_000 * n) // 20_005


@functools.lru_cache(maxsize=None)
def masks(n, dims):
    """name -> the rows that pass (bool[n]). Chunks are the mirror form's."""
    c = MIRROR_CHUNK[dims]
    rng = np.random.default_rng(STORE_SEED + 1)
    out = {}
    out["r15"] = rng.random(n) >= 1.0 / 16.0
    out["half"] = rng.random(n) < 0.5
    lo, hi = range_bounds(n)
    out["range"] = np.zeros(n, dtype=bool)
    out["range"][lo:hi] = True
    one = np.zeros(n, dtype=bool)
    for first in range(0, n, c):                       # exactly one passing row in every chunk, the ragged last one included
        one[first + rng.integers(0, min(c, n - first))] = True
    out["one_per_chunk"] = one
    tail0 = n - (n % c or c)                           # first row of the final (partial) chunk
    tail = np.zeros(n, dtype=bool)
    tail[tail0:] = True
    tail[rng.choice(tail0, 65, replace=False)] = True
    out["tail_plus_65"] = tail
    for m in (65, 64):
        few = np.zeros(n, dtype=bool)
        few[rng.choice(n, m, replace=False)] = True
        out["m%d" % m] = few
    out["m0"] = np.zeros(n, dtype=bool)
    for v in out.values():
        v.setflags(write=False)
    return out


def flags_for(n, dims):
    """The flag column that carries every mask but "range" (a time range on ts = row): a row FAILS mask `name` iff MASK_BIT[name] is set."""
    fl = np.zeros(n, dtype=np.uint32)
    for name, bit in MASK_BIT.items():
        fl[~masks(n, dims)[name]] |= np.uint32(bit)
    return fl


def mirror_of(metric, rows):
    """What the conversion kernel stores, widened back to f32: cosine rows scaled by 1 / their f32 norm and rounded to bf16
    (rows of norm <= 1e-6 zeroed), dot rows rounded as they are; and max ||x - bf16(x)|| over the rows, x the row that was rounded."""
    x = rows
    if metric == COS:
        n = np.sqrt(np.sum(rows * rows, axis=1, dtype=np.float32))
        with np.errstate(divide="ignore"):
            scale = np.where(n > np.float32(1e-6), np.float32(1.0) / n, np.float32(0.0)).astype(np.float32)
        x = (rows * scale[:, None]).astype(np.float32)
    m = bf16_rne(x)
    err = np.linalg.norm(x.astype(np.float64) - m.astype(np.float64), axis=1)
    return m, float(err.max())


def finish_eps(metric, dims, q_norm, max_norm, max_row_err, use_measured=True):
    """eps of the certificate, written out from Bf16Eps in mirror_finish.h (step 5 of mirror_finish): its doubles, its constants, its final round up to f32."""
    qn = 1.0 + 1e-6 if metric == COS else float(q_norm)
    vn = 1.0 + 1e-6 if metric == COS else float(max_norm)
    u = 0.0078125 * (1.0 + 1.0 / 512.0) + dims * 5.97e-8 + 1e-6
    dot_err = u * qn * vn * 1.001
    if use_measured and max_row_err > 0.0:
        measured = qn * float(np.float32(max_row_err)) * 1.001 + 3.0 * dims * 5.97e-8 * qn * vn
        dot_err = min(dot_err, measured)
    eps = dot_err + 3e-6 if metric == COS else dot_err + 1e-6 * (1.0 + qn * vn)
    return float(np.nextafter(np.float32(eps), np.float32(np.inf)))


class Model:
    """Approximate and exact distances of every (row, query) of one store in float64, and the store's eps per query."""

    def __init__(self, metric, rows, qs):
        self.metric, self.dims = metric, rows.shape[1]
        r64, q64 = rows.astype(np.float64), qs.astype(np.float64)
        qn = np.linalg.norm(q64, axis=1)
        mirror, max_row_err = mirror_of(metric, rows)
        dots = r64 @ q64.T
        approx = mirror.astype(np.float64) @ q64.T
        if metric == COS:
            rn = np.linalg.norm(r64, axis=1)
            with np.errstate(divide="ignore", invalid="ignore"):
                self.exact = 1.0 - np.where(rn[:, None] > 1e-6, dots / (rn[:, None] * qn[None, :]), 0.0)
            self.approx = 1.0 - approx / qn[None, :]
        else:
            self.exact = 1.0 - dots
            self.approx = 1.0 - approx
        max_norm = float(np.linalg.norm(r64, axis=1).max())
        self.eps = np.array([finish_eps(metric, self.dims, float(np.float32(n_)), max_norm, max_row_err) for n_ in qn])

    def margin(self, mask, q, k):
        """a_64 - eps - d_k over the passing rows; -inf when 64 or fewer pass (the form is not taken)."""
        if int(mask.sum()) <= MIRROR_KP:
            return -np.inf
        a = np.partition(self.approx[mask, q], MIRROR_KP - 1)[MIRROR_KP - 1]
        d = np.partition(self.exact[mask, q], k - 1)[k - 1]
        return float(a - self.eps[q] - d)


@functools.lru_cache(maxsize=None)
def model(name):
    metric, _, dims = STORES[name]
    return Model(metric, store_rows(name), queries(dims))


def takes_mirror_form(metric, dims, k, m, mode=2, variant=0, grid_blocks=0):
    """The host's rule for a query the route rule has already sent to the masked scan (filter_host.inc), for "predicate_mirror" 2."""
    return (mode == 2 and metric in (COS, DOT) and dims in MIRROR_CHUNK and 1 <= k <= MIRROR_MAX_K and variant == 0 and
            grid_blocks <= 512 and m > MIRROR_KP)


# ---- the store of exact duplicates (the period-256 pattern) ----
DUP_ROWS, DUP_DIMS, DUP_PASSING = 20_005, 384, 256 * 70      # rows [0, 17 920) pass: 70 copies of each of the 256 distinct rows


@functools.lru_cache(maxsize=None)
def dup_rows():
    x = oracle.tie_pattern(0, DUP_ROWS, DUP_DIMS)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def dup_model():
    return Model(COS, dup_rows(), queries(DUP_DIMS))


def dup_mask():
    m = np.zeros(DUP_ROWS, dtype=bool)
    m[:DUP_PASSING] = True
    return m
