"""Top-k selection held to an exact model on distances the test controls bit for bit. No engine code runs here:
test_selection_edges_cpu.py proves what each construction must have for its GPU test to be able to fail,
test_selection_edges_gpu.py asserts the model's answer on the device, bit for bit, on every selection route.

Why the distances are exact. Under the dot metric with a one-hot query e_j the kernels' fma chains add exact zeros to 1 * v[j] (every
other element of the row is finite), so a row's distance is f32(1) - v[j]: ONE IEEE f32 subtraction, whatever kernel computes it
(row_math.h). Column j of a store therefore IS a distance array, and one store carries several. Under l2 with a zero query and rows
x * e_0 the distance is f32(x * x); under cosine with rows +-2^e * e_0 and q = e_0 it is 0, 2, or 1 (a zero row, or a row whose norm
is at or below the 1e-6 floor of CosineDistance.metal:323, which the engine and oracle/wax_oracle.c:178 both score as similarity 0).

The model (`Column.answer`): f32 distance bits -> order_bits -> lexsort by (key, global row) -> the first min(clamp(k), n) ->
non-finite distances dropped (MetalVectorEngine.swift:597, wax_oracle.c:322) -> score, frame id. `radix_select` restates the 8-pass
radix selection of kernels.hip (select_hist_kernel / select_compact_kernel) with its loop structure, so that the CPU test can say
which pass decides a case and which cases a given defect of those kernels would change."""
import numpy as np

ONE = np.float32(1.0)
MAX_RESULTS = 10000
N_BIG = 70001                                  # = 1 mod 4, >= 256 * 193, > 65 536
SMALL_NS = (193, 257, 1023)
ROW_BASES = (0, 0x00FFFF00, 0xFFFE0000)
KS = (1, 10, 64, 65, 192, 193, 257, 1000, 4096, 10000)
COS_NORM_FLOOR = np.float32(1e-6)


def clamp_topk(k):
    return max(1, min(int(k), MAX_RESULTS))


def order_bits(d):
    """common.h order_bits: signed integer order == float order."""
    b = np.ascontiguousarray(d, dtype=np.float32).view(np.int32)
    return b ^ ((b >> 31) & 0x7fffffff)


def canonical(d):
    """finish_distance's last two lines: NaN -> +inf, -0 -> +0."""
    d = np.array(d, dtype=np.float32)
    d[np.isnan(d)] = np.inf
    return (d + np.float32(0.0)).astype(np.float32)


def dot_distance(x):
    with np.errstate(all="ignore"):
        return canonical(ONE - np.asarray(x, dtype=np.float32))


def l2_distance(x):
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(all="ignore"):
        return canonical(x * x)


def cosine_distance(x):
    """Rows x * e_0 against q = e_0: sqrt(x * x) > 1e-6 ? 1 - x / |x| : 1 (CosineDistance.metal:321-325; wax_oracle.c:176-179)."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(all="ignore"):
        vn = np.sqrt(x * x).astype(np.float32)
        sim = np.where(vn > COS_NORM_FLOOR, x / vn, np.float32(0.0)).astype(np.float32)
    return canonical(ONE - sim)


def ukeys(d, row_base):
    """ukey_of: (ordered distance : global row), unsigned-ordered."""
    ob = order_bits(d).astype(np.int64).astype(np.uint64) & np.uint64(0xffffffff)
    rows = np.uint64(row_base) + np.arange(len(d), dtype=np.uint64)
    assert int(rows[-1]) < 2 ** 32
    return ((ob ^ np.uint64(0x80000000)) << np.uint64(32)) | rows


def frame_ids(n):
    return (np.arange(n, dtype=np.uint64) + np.uint64(1)) * np.uint64(1_000_003)


class Column:
    """One distance array and the model's answers over it."""

    def __init__(self, name, metric, x, d, ids=None):
        self.name, self.metric = name, metric
        self.x = np.ascontiguousarray(x, dtype=np.float32)
        self.d = np.ascontiguousarray(d, dtype=np.float32)
        self.n = len(self.d)
        self.ids = frame_ids(self.n) if ids is None else ids
        self._order = {}

    def order(self, row_base):
        if row_base not in self._order:
            rows = np.uint64(row_base) + np.arange(self.n, dtype=np.uint64)
            self._order[row_base] = np.lexsort((rows, order_bits(self.d)))      # by (key, global row)
        return self._order[row_base]

    def taken(self, k, row_base=0):
        """Local rows of the first min(clamp(k), n) keys, ascending by key (non-finite distances still in)."""
        return self.order(row_base)[:min(clamp_topk(k), self.n)]

    def answer(self, k, row_base=0):
        """(ids, scores) exactly as searchArrays must return them."""
        rows = self.taken(k, row_base)
        rows = rows[np.isfinite(self.d[rows])]
        d = self.d[rows]
        scores = (ONE - d) if self.metric == 0 else -d
        return self.ids[rows], scores.astype(np.float32)

    def tie_group(self, k, row_base=0):
        """(first rank, last rank), 1-based, of the rows whose distance equals the k-th's: it straddles rank k when last > k."""
        kk = min(clamp_topk(k), self.n)
        ob = order_bits(self.d)[self.order(row_base)]
        return int(np.searchsorted(ob, ob[kk - 1], "left")) + 1, int(np.searchsorted(ob, ob[kk - 1], "right"))

    def deciding_pass(self, k, row_base=0):
        """The radix pass after which nothing is left to decide, from the sorted keys alone: the first pass p such that every key
        sharing digits 0..p with the k-th key is among the k smallest (the kernel's `all_needed`), else 7."""
        kk = min(clamp_topk(k), self.n)
        u = np.sort(ukeys(self.d, row_base))
        kth = int(u[kk - 1])
        for p in range(8):
            shift = 56 - 8 * p
            hi = kth | ((1 << shift) - 1)
            if int(np.searchsorted(u, np.uint64(hi), "right")) == kk:
                return p
        raise AssertionError("keys are unique: pass 7 always decides")


# ---- the radix selection of kernels.hip, restated --------------------------------------------------------------------------------

def select_grid_for(n, cap=0):
    g = min(2048, (n + 255) // 256)
    return min(g, cap) if cap > 0 else g


def hist_loops(n, grid):
    """For every float4 f of the distance array: which loop of select_hist_kernel counts it (4 = four in flight, 2 = two, 1 = the
    single-trip loop) and the float4 index the four-deep loop's trip STARTS at (`i4`; the correct row index uses `j4 = i4 + j * stride`)."""
    n4, stride = n // 4, grid * 256
    f = np.arange(n4, dtype=np.int64)
    t, trip = f % stride, f // stride
    trips = (n4 - t + stride - 1) // stride                         # float4s of thread t
    in4 = trip < 4 * (trips // 4)
    rest = trips % 4
    in2 = ~in4 & (rest >= 2) & (trip - 4 * (trips // 4) < 2)
    loop = np.where(in4, 4, np.where(in2, 2, 1))
    i4 = np.where(in4, t + (trip - trip % 4) * stride, f)
    return loop, i4


def compact_loops(n, grid):
    n4, stride = n // 4, grid * 256
    f = np.arange(n4, dtype=np.int64)
    t, trip = f % stride, f // stride
    trips = (n4 - t + stride - 1) // stride
    return np.where(trip < 2 * (trips // 2), 2, 1)


DEFECTS = ("no_tail", "no_all_needed", "all_needed_zeros", "no_prefix_match", "four_deep_i4")


def radix_select(d, row_base, k, grid_cap=0, defect=None):
    """select_hist_kernel x 8 + select_compact_kernel + rank sort on the CPU. Returns (sorted selected signed-order keys or None when
    the compaction does not find exactly k keys, the pass that set the final threshold, whether by `all_needed`).
    `defect`: None = the kernels as they are; else one line of them reverted —
      no_tail            the `n % 4` tail of select_hist_kernel is not counted
      no_all_needed      the early exit is never taken (the threshold is always the exact k-th key, after pass 7)
      all_needed_zeros   the early exit's threshold keeps zeros, not ones, below the decided digits
      no_prefix_match    `(u >> (shift + 8)) == prefix` always true
      four_deep_i4       the four-in-flight loop numbers its rows from `4 * i4` instead of `4 * j4`"""
    assert defect is None or defect in DEFECTS
    d = np.ascontiguousarray(d, dtype=np.float32)
    n = len(d)
    k = int(k)
    assert 1 <= k <= min(n, MAX_RESULTS)
    grid = select_grid_for(n, grid_cap)
    true_u = ukeys(d, row_base)
    u = true_u.copy()
    live = np.ones(n, dtype=bool)
    if defect == "four_deep_i4":
        loop, i4 = hist_loops(n, grid)
        idx = np.arange(n)
        n44 = (n // 4) * 4
        wrong_row = np.where(np.repeat(loop, 4) == 4, np.repeat(4 * i4, 4) + idx[:n44] % 4, idx[:n44])
        u[:n44] = (true_u[:n44] & np.uint64(0xffffffff00000000)) | (np.uint64(row_base) + wrong_row.astype(np.uint64))
    if defect == "no_tail":
        live[(n // 4) * 4:] = False
    prefix, rem, thr, decided, by_all = 0, k, None, None, False
    for p in range(8):
        shift = 56 - 8 * p
        match = live.copy()
        if p > 0 and defect != "no_prefix_match":
            match &= (u >> np.uint64(shift + 8)) == np.uint64(prefix)
        hist = np.bincount(((u[match] >> np.uint64(shift)) & np.uint64(0xff)).astype(np.int64), minlength=256)
        cum = np.concatenate(([0], np.cumsum(hist)[:-1]))
        pick = np.nonzero((cum < rem) & (cum + hist >= rem))[0]
        if len(pick) != 1:
            return None, p, False                                    # no thread picks: the state stays undecided
        b = int(pick[0])
        left = rem - int(cum[b])
        np_ = (prefix << 8) | b
        all_needed = left == int(hist[b]) and defect != "no_all_needed"
        if p == 7 or all_needed:
            fill = 0 if (defect == "all_needed_zeros" and p < 7) else (1 << shift) - 1
            thr, decided, by_all = (np_ << shift) | fill, p, all_needed
            break
        prefix, rem = np_, left
    sel = true_u[true_u <= np.uint64(thr)]
    if len(sel) != k:
        return None, decided, by_all
    return np.sort(sel), decided, by_all


def model_keys(col, k, row_base):
    return np.sort(ukeys(col.d, row_base))[:min(clamp_topk(k), col.n)]


# ---- constructions ---------------------------------------------------------------------------------------------------------------

def _f32_from_bits(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def _ladder(rng, n, first_bits, count, block_end_bits):
    """`count` consecutive f32 values upward from first_bits with random multiplicities (about a sixth of the rows in all, at least
    one row each); every other row takes one of the values above the ladder up to block_end_bits (inclusive) — the last values of
    the ladder's own 256-value block, so the whole column shares its leading key bytes. Shuffled."""
    vals = _f32_from_bits(first_bits + np.arange(count, dtype=np.uint32))
    budget = max(count, n // 6)
    mult = 1 + rng.multinomial(budget - count, np.ones(count) / count)
    rest = _f32_from_bits(np.arange(first_bits + count, block_end_bits + 1, dtype=np.uint32))
    assert len(rest) >= 8
    d = np.concatenate([np.repeat(vals, mult), rng.choice(rest, n - int(mult.sum()))]).astype(np.float32)
    assert len(d) == n
    return d[rng.permutation(n)]


def dot_columns(n, seed=20261, intended=None):
    """name -> x (f32 [n]) for the dot stores; d = f32(1) - x. The ladders are given as d and x derived as f32(1) - d; `intended`
    (a dict, if given) receives those d arrays as they were meant, for `check_round_trip`."""
    rng = np.random.default_rng(seed + n)
    cols = {}
    cols["flat"] = np.full(n, 0.25, dtype=np.float32)
    for g in (200, 300, 66000):
        if g >= n:
            g_eff = n // 2 if g < 66000 else None                   # small stores: half the rows; no 66 000 there
        else:
            g_eff = g
        if g_eff is None:
            continue
        x = np.full(n, 0.25, dtype=np.float32)
        x[rng.choice(n - 1, g_eff - 1, replace=False)] = 0.5
        x[n - 1] = 0.5                                              # the last row (in the `n % 4` tail) belongs to the lower group
        cols[f"straddle-{g}"] = x
    cnt = lambda c: min(c, max(8, n // 8))                                           # noqa: E731  (small stores: shorter ladders)
    lad = {
        "ladder-low-byte": _ladder(rng, n, 0x3F400000, cnt(200), 0x3F4000FF),                 # passes 0-2 one bin, pass 3 decides
        "ladder-carry": _ladder(rng, n, 0x3F400000 - cnt(300) // 2, cnt(300), 0x3F4000FF),    # ...3FFFFF | 400000...: a carry through three bytes
        "ladder-exponent": _ladder(rng, n, 0x3F800000 - cnt(300) // 2, cnt(300), 0x3F8000FF),  # straddles 1.0: an exponent change
    }
    for name, d in lad.items():
        cols[name] = (ONE - d).astype(np.float32)
        if intended is not None:
            intended[name] = d
    z = np.array([-2.0 ** -20, -2.0 ** -21, -2.0 ** -22, -2.0 ** -23, 0.0, 2.0 ** -24, 2.0 ** -23, 3 * 2.0 ** -24, 2.0 ** -22,
                  2.0 ** -21, 2.0 ** -20], dtype=np.float32)
    mult = 1 + rng.multinomial(max(len(z), n // 20) - len(z), np.ones(len(z)) / len(z))
    d = np.concatenate([np.repeat(z, mult), rng.uniform(0.5, 0.9, n - int(mult.sum())).astype(np.float32)])[rng.permutation(n)]
    cols["around-zero"] = (ONE - d).astype(np.float32)
    if intended is not None:
        intended["around-zero"] = d
    e = np.arange(-126, 128)
    pool = np.concatenate([2.0 ** e, -(2.0 ** e), [0.0, -0.0], [2.0 ** -127, -2.0 ** -130, 2.0 ** -149, -2.0 ** -149, 3 * 2.0 ** -140]])
    pool = pool.astype(np.float32)
    cols["wide"] = np.concatenate([pool, rng.choice(pool, max(0, n - len(pool)))])[:n][rng.permutation(n)].astype(np.float32)
    return cols


LADDERS = ("ladder-low-byte", "ladder-carry", "ladder-exponent", "around-zero")


def check_round_trip(x, d_intended, ctx):
    """x was derived as f32(1) - d from the d the construction meant: the distance the kernels form, f32(1) - x, must be that d bit
    for bit — else the column holds other values than the ladder it claims."""
    d_intended = np.ascontiguousarray(d_intended, dtype=np.float32)
    assert not np.any(np.isnan(d_intended)) and not np.any(np.signbit(d_intended) & (d_intended == 0)), ctx
    got = dot_distance(x)
    assert np.array_equal(got.view(np.uint32), d_intended.view(np.uint32)), ctx


# where each distribution sits in a 64-d row (the other columns are finite junk, so a wrong row stride still shows)
DOT64_COLUMNS = {"flat": 0, "straddle-200": 3, "straddle-300": 17, "straddle-66000": 21, "ladder-low-byte": 34, "ladder-carry": 40,
                 "ladder-exponent": 47, "around-zero": 58, "wide": 63}
# 5-d rows hold five distributions: two stores
DOT5_COLUMNS = ({"flat": 0, "straddle-200": 1, "straddle-66000": 2, "ladder-carry": 3, "wide": 4},
                {"straddle-300": 0, "ladder-low-byte": 1, "ladder-exponent": 2, "around-zero": 3})


def dot_store(n, dims, placement, seed=20261):
    """(rows f32 [n, dims], {name: (column, Column)}): the named distributions at their columns, N(0, 1) junk everywhere else."""
    cols = dot_columns(n, seed)
    rows = np.random.default_rng(seed + 1000 + dims).standard_normal((n, dims)).astype(np.float32)
    out = {}
    for name, j in placement.items():
        if name not in cols:
            continue
        rows[:, j] = cols[name]
        out[name] = (j, Column(name, 1, cols[name], dot_distance(cols[name])))
    assert np.all(np.isfinite(rows))
    return np.ascontiguousarray(rows), out


def one_hot(dims, j):
    q = np.zeros(dims, dtype=np.float32)
    q[j] = 1.0
    return q


NON_FINITE_N = 1027
NON_FINITE_WINNERS, NON_FINITE_PLUS_INF, NON_FINITE_NAN = 7, 5, 5
NON_FINITE_NAN_ROWS = (1003, 1008, 1013, 1019, 1024)      # beyond row 1 000: see test_selection_edges_cpu.py on the oracle's heap


def non_finite_store(dims=64, seed=20262):
    """Column 0 only is special, every other column finite: 7 rows x = +inf (d = -inf: they win a slot each and are dropped), 5 rows
    x = -inf (d = +inf), 5 rows NaN (-> +inf). 1 010 finite rows: k <= 1 000 returns k - 7, k = n returns n - 17."""
    rng = np.random.default_rng(seed)
    n = NON_FINITE_N
    rows = rng.standard_normal((n, dims)).astype(np.float32)
    x = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    free = np.setdiff1d(np.arange(1, n), NON_FINITE_NAN_ROWS)
    pick = rng.choice(free, NON_FINITE_WINNERS + NON_FINITE_PLUS_INF, replace=False)
    x[pick[:NON_FINITE_WINNERS]] = np.inf
    x[pick[NON_FINITE_WINNERS:]] = -np.inf
    x[list(NON_FINITE_NAN_ROWS)] = np.nan
    rows[:, 0] = x
    assert np.all(np.isfinite(rows[:, 1:]))
    return np.ascontiguousarray(rows), Column("non-finite", 1, x, dot_distance(x))


L2_ZEROS, L2_UNDERFLOW, L2_SUBNORMAL_EACH, L2_INF = 90, 60, 20, 9
L2_SUBNORMAL_EXPONENTS = tuple(range(-70, -63))              # x = 2^e: d = 2^-140 .. 2^-128, all below the smallest normal 2^-126


def l2_store(n, dims=64, seed=20263):
    """Rows x * e_0 for a zero query, d = f32(x * x): 90 true zero rows and 60 rows x = +-2^-80 (x * x underflows to 0: one tie group
    of 150), 20 rows at each of 2^-70 .. 2^-64 (subnormal d, ranks 151 .. 290), 9 rows 2^64 (d = +inf, dropped), ordinary values."""
    rng = np.random.default_rng(seed + n)
    special = np.concatenate([np.zeros(L2_ZEROS), np.full(L2_UNDERFLOW // 2, 2.0 ** -80), np.full(L2_UNDERFLOW // 2, -2.0 ** -80),
                              np.repeat(2.0 ** np.array(L2_SUBNORMAL_EXPONENTS, dtype=np.float64), L2_SUBNORMAL_EACH),
                              np.full(L2_INF, 2.0 ** 64)])
    x = np.concatenate([special, rng.uniform(0.1, 2.0, n - len(special)) * rng.choice([-1.0, 1.0], n - len(special))]).astype(np.float32)
    x = x[rng.permutation(n)]
    rows = np.zeros((n, dims), dtype=np.float32)
    rows[:, 0] = x
    return rows, Column("l2", 2, x, l2_distance(x))


L2_RANKS = (L2_ZEROS + L2_UNDERFLOW - 1, L2_ZEROS + L2_UNDERFLOW, L2_ZEROS + L2_UNDERFLOW + 1,
            L2_ZEROS + L2_UNDERFLOW + 7 * L2_SUBNORMAL_EACH, L2_ZEROS + L2_UNDERFLOW + 7 * L2_SUBNORMAL_EACH + 1)


def cosine_store(n, dims=64, seed=20264):
    """Rows +-2^e * e_0 (|e| <= 60) and zero rows, q = e_0: 40 % of the rows at d = 0, 30 % at d = 1, 30 % at d = 2 by the MODEL's
    count — a row of norm <= 1e-6 (e <= -20) scores similarity 0 like a zero row (CosineDistance.metal:323, wax_oracle.c:178), so the
    d = 1 level is made of true zero rows and of such tiny rows of either sign. Returns (rows, Column, (n0, n1))."""
    rng = np.random.default_rng(seed + n)
    n0, n1 = (4 * n) // 10, (3 * n) // 10
    n2 = n - n0 - n1
    big = lambda m: 2.0 ** rng.integers(-19, 61, m)                                  # noqa: E731  norm above the floor
    tiny = n1 // 3
    level1 = np.concatenate([np.zeros(n1 - tiny), 2.0 ** rng.integers(-60, -19, tiny) * rng.choice([-1.0, 1.0], tiny)])
    x = np.concatenate([big(n0), level1, -big(n2)]).astype(np.float32)[rng.permutation(n)]
    rows = np.zeros((n, dims), dtype=np.float32)
    rows[:, 0] = x
    return rows, Column("cosine", 0, x, cosine_distance(x)), (n0, n1)


def cosine_ranks(n0, n1):
    return (n0 - 1, n0, n0 + 1, n0 + n1 - 1, n0 + n1, n0 + n1 + 1)


def ks_for(col_name, n):
    """Every k a (store, column) is queried at: the matrix, the straddle columns' own G - 1, G, G + 1, and n, n + 1 on the small stores."""
    ks = list(KS)
    if col_name.startswith("straddle-"):
        g = int(col_name.split("-")[1])
        g = g if g < n else n // 2
        ks += [g - 1, g, g + 1]
    if n <= 1027:
        ks += [n, n + 1]
    return sorted(set(ks))


def row_bases_for(n):
    return [rb for rb in ROW_BASES if rb + n <= 2 ** 32]


# the one default-grid case
BIG_N, BIG_FORCED = 6_291_463, 300_000


def big_default_grid_loops():
    """(rows counted by the four-deep loop, by the two-deep loop, by the tail) of select_hist_kernel at BIG_N rows and 2 048 workgroups."""
    grid = select_grid_for(BIG_N)
    loop, _ = hist_loops(BIG_N, grid)
    return grid, int(np.sum(loop == 4)) * 4, int(np.sum(loop == 2)) * 4, BIG_N % 4


# ---- the stores both test files use --------------------------------------------------------------------------------------------

STORE_NAMES = ("dot-70001x64", "dot-70001x5-a", "dot-70001x5-b", "dot-193x64", "dot-257x64", "dot-1023x64", "non-finite-1027x64",
               "l2-70001x64", "l2-1023x64", "cosine-1023x64", "cosine-14003x64")
SMALL_COLUMNS = {name: j for name, j in DOT64_COLUMNS.items() if name != "straddle-66000"}   # (66 000 rows do not fit)


def build_store(name):
    """-> (metric, rows f32 [n, dims], {column name: (query, Column, extra ks)})."""
    kind, shape = name.split("-", 1) if not name.startswith("non-finite") else ("non-finite", name[len("non-finite-"):])
    parts = shape.split("-")
    n, dims = (int(v) for v in parts[0].split("x"))
    if kind == "dot":
        placement = DOT64_COLUMNS if dims == 64 and n == N_BIG else SMALL_COLUMNS if dims == 64 else DOT5_COLUMNS["ab".index(parts[1])]
        rows, cols = dot_store(n, dims, placement)
        return 1, rows, {c: (one_hot(dims, j), col, ()) for c, (j, col) in cols.items()}
    if kind == "non-finite":
        rows, col = non_finite_store(dims)
        return 1, rows, {"non-finite": (one_hot(dims, 0), col, (n,))}
    if kind == "l2":
        rows, col = l2_store(n, dims)
        return 2, rows, {"l2": (np.zeros(dims, dtype=np.float32), col, L2_RANKS)}
    rows, col, (n0, n1) = cosine_store(n, dims)
    return 0, rows, {"cosine": (one_hot(dims, 0), col, cosine_ranks(n0, n1))}


def ks_of(col_name, col, extra=()):
    return sorted(set(ks_for(col_name, col.n)) | set(int(k) for k in extra))

# column names per store, without building anything (test ids)
STORE_COLUMNS = {"dot-70001x64": tuple(DOT64_COLUMNS), "dot-70001x5-a": tuple(DOT5_COLUMNS[0]), "dot-70001x5-b": tuple(DOT5_COLUMNS[1]),
                 "dot-193x64": tuple(SMALL_COLUMNS), "dot-257x64": tuple(SMALL_COLUMNS), "dot-1023x64": tuple(SMALL_COLUMNS),
                 "non-finite-1027x64": ("non-finite",), "l2-70001x64": ("l2",), "l2-1023x64": ("l2",), "cosine-1023x64": ("cosine",),
                 "cosine-14003x64": ("cosine",)}
assert tuple(STORE_COLUMNS) == STORE_NAMES


# ---- search_internal.inc's rule for trying the short selection at k > 192 (kernels.hip: short_depth, select_short_viable) ------

def short_depth(k, lists, per_list):
    return min(max((2 * k + lists - 1) // lists, 4), per_list)


def select_short_viable(k, lists, per_list):
    if lists <= 0 or k < 1 or per_list < 1 or lists * short_depth(k, lists, per_list) > 16384:
        return False
    return k <= per_list or 3 * k <= lists * per_list


def tries_short(k_eff, n, scan_grid):
    per_list = 64 if k_eff <= scan_grid * 8 else 192
    return k_eff > 192 and select_short_viable(k_eff, scan_grid, per_list) and n >= 256 * k_eff


# kernels.h: which fused scans merge in their own kernel; search_internal.inc (enqueue_scan, enqueue_list_merge): what follows the others
SCAN_FUSE_MERGE_GRID, SCAN_KWAY_MAX_K, SCAN_KWAY_MERGE_GRID, SCAN_KWAY_MAX_BYTES, FUSED_MAX_K = 160, 64, 512, 2 << 30, 192


def scan_merges_in_kernel(grid, k, n, dims):
    return grid <= SCAN_FUSE_MERGE_GRID or (k <= SCAN_KWAY_MAX_K and grid <= SCAN_KWAY_MERGE_GRID and n * dims * 4 <= SCAN_KWAY_MAX_BYTES)


def expected_route(k_eff, n, dims, scan_grid, select_short, force_general):
    """(short selections enqueued, scans that merged in their own kernel) by ONE blocking single query under default tuning but for
    the two keys given: the deltas of "short_selects" and "merged_scans"."""
    if force_general or k_eff > FUSED_MAX_K:                         # distance pass + radix selection, the short selection in front of it
        return (1 if select_short and not force_general and tries_short(k_eff, n, scan_grid) else 0), 0
    if scan_merges_in_kernel(scan_grid, k_eff, n, dims):
        return 0, 1
    # a second launch merges the lists: the short merge for 64 < k <= 192 (lists of k entries), else the wave-list merge
    return (1 if select_short and k_eff > SCAN_KWAY_MAX_K and select_short_viable(k_eff, scan_grid, k_eff) else 0), 0
