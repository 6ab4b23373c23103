"""The twin store, its sweep and the float64 model behind tests/test_batch_positions_cpu.py and tests/test_batch_positions_gpu.py.

Every test that reaches the batched pipelines (batch.hip: the filtering GEMM batch_gemm_rq_kernel, the LDS-tiled batch_gemm_kernel, the
slab pipeline; multiscan.hip: the shared exact pass) checks every QUERY of a batch, on corpora where an answer needs a fraction of a
percent of the rows: a row the filter never scores, or scores from another row's bytes, only has to lose — and it does. The certificate
 cannot tell either: "a row not among the candidates has approximate distance >= a_max" assumes the filter saw the row.

The twin store makes every row POSITION required. N rows, H = N // 2:
  rows 0 .. H-1      seeded Gaussian unit rows
  row  i + H         unit(row_i + SIGMA * g_i), g_i Gaussian with E|g_i|^2 = 1: cosine 1 / sqrt(1 + SIGMA^2) ~ 0.95 with row i
  row  N-1, N odd    a lone Gaussian unit row (its query is checked at rank 1 only)
  dot                every row times DOT_SCALE (one common scale: the self row still wins); cosine and L2: unit rows.
The sweep: the stored rows themselves, bit copies, in store order, in batches of nq (the last one ragged), top_k = 2. Query i expects
ids [i, partner(i)], count 2, the self score and the pair's score — from the rows alone, O(N D) in float64 (`expected`).

H is never a multiple of (tile rows x workgroups of a query group) — `stride_rows`, restated from batch.hip below; the CPU test
asserts it for every case — so a row and its twin sit in different tiles, at different places of them, in different workgroups and,
where the filtering GEMM has a tail pool, on both sides of its first tile for a part of the pairs (`pool_first_row`).

What makes the GPU sweeps able to fail is shown by the CPU test on these definitions: (a) `pair_cosines` in [0.90, 0.99]; (b) no
stranger outranks a twin — `stranger_best` directly on the smallest store of each dimension, `cap_bound` on the others; (c)
`certificate_margins`: the 64th best approximate distance less the worst-case eps less the exact second distance stays far above
zero, so no fallback is ever owed to the certificate; (d) `drop_row`: a filter that loses one row position changes exactly that row's
own answer and its twin's.

The geometry restated here (tile rows, workgroups per group, the pool) decides no expected answer: only where the sample of
bit-compared rows is taken and what the CPU test asserts about H."""
import math

import numpy as np

COS, DOT, L2 = 0, 1, 2
METRIC_NAME = {COS: "cosine", DOT: "dot", L2: "l2"}
SIGMA = 0.33
DOT_SCALE = 1.7
K = 2
KP = 64                               # batch_kp(2, .): k' = max(64, 2 k + 32) approximate candidates per query
STORE_SEED = 20261105
PAIR_COS_MIN, PAIR_COS_MAX = 0.90, 0.99
CAP_T, CAP_SUM_MAX = 0.8, 1e-3
MARGIN_MIN = 0.3                      # (c), in units of the cosine distance (x DISTANCE_UNIT of the metric)
MARGIN_SAMPLE = 256

# ---- geometry of the filters (batch.hip), restated ------------------------------------------------------------------------------------
RQ_DIMS = (128, 256, 384, 512, 768)   # register-resident-queries GEMM: cosine / dot at these dimensions
GN = 128                              # rows per tile of the LDS-tiled kernel
GROUP_QUERIES = 256                   # queries per query group of the rq GEMM
WORKGROUPS = 256                      # its persistent workgroups, over all groups
DYN_MIN_TILES = 24                    # tail pool: at least this many tiles per workgroup, one query group
MAX_BATCH = 1024                      # kBatchMaxQ


def is_rq(metric, dims):
    return metric != L2 and dims in RQ_DIMS


def tile_rows(metric, dims):
    if not is_rq(metric, dims):
        return GN
    return 128 if dims == 128 else 32 if dims == 768 else 64


def n_tiles(metric, dims, n):
    return -(-n // tile_rows(metric, dims))


def query_groups(nq):
    return -(-min(nq, MAX_BATCH) // GROUP_QUERIES)


def workgroups_per_group(metric, dims, n, nq):
    """rq_geometry: 256 workgroups shared out over the query groups, clipped to the tile count. The LDS-tiled kernel gives every tile
    a workgroup of its own: 1."""
    if not is_rq(metric, dims):
        return 1
    return max(1, min(WORKGROUPS // query_groups(nq), n_tiles(metric, dims, n)))


def stride_rows(metric, dims, n, nq):
    """Rows between two tiles of one workgroup's fixed share: tile rows x workgroups of the group."""
    return tile_rows(metric, dims) * workgroups_per_group(metric, dims, n, nq)


def pool_first_row(metric, dims, n, nq):
    """First row of the tail pool of the filtering GEMM, or None where there is none (more than one query group, fewer than 24 tiles
    per workgroup, another kernel): positions below n_static = tiles_min - max(tiles_min // 12, 4) are fixed shares."""
    if not is_rq(metric, dims) or query_groups(nq) != 1:
        return None
    per_group = workgroups_per_group(metric, dims, n, nq)
    tiles_min = n_tiles(metric, dims, n) // per_group
    if tiles_min < DYN_MIN_TILES:
        return None
    n_static = tiles_min - max(tiles_min // 12, 4)
    return n_static * per_group * tile_rows(metric, dims)


# ---- the cases of the GPU sweeps ------------------------------------------------------------------------------------------------------
# (id, route, metric, dims, rows, queries per batch, tuning keys set for the sweep, two batches in flight)
POOL, FIXED, GROUPS, SPLIT, TILED, SLAB, EXACT, HANDLE = "pool", "fixed", "groups", "split", "tiled", "slab", "exact", "handle"
N_POOL_384, N_POOL_768 = 24 * 256 * 64 + 37, 24 * 256 * 32 + 19
N_MID, N_CLIP, N_TILED, N_SLAB, N_FLOOR, N_EXACT = 40_037, 4_099, 65_536 + 77, 20_011, 3_001, 5_003


def _case(cid, route, metric, dims, n, nq=256, tuning=(), pipelined=False):
    return {"id": cid, "route": route, "metric": metric, "dims": dims, "n": n, "nq": nq, "tuning": tuple(tuning), "pipelined": pipelined}


CASES = [
    _case("pool-cos384", POOL, COS, 384, N_POOL_384),
    _case("pool-cos768", POOL, COS, 768, N_POOL_768),
    _case("fixed-cos128", FIXED, COS, 128, N_MID),
    _case("fixed-cos256", FIXED, COS, 256, N_MID, pipelined=True),
    _case("fixed-cos384", FIXED, COS, 384, N_MID),
    _case("fixed-cos512", FIXED, COS, 512, N_MID, pipelined=True),
    _case("fixed-cos768", FIXED, COS, 768, N_MID),
    _case("fixed-dot384", FIXED, DOT, 384, N_MID),
    _case("clipped-cos384", FIXED, COS, 384, N_CLIP),
    _case("groups2-cos384", GROUPS, COS, 384, N_MID, nq=512),
    _case("groups3-cos384", GROUPS, COS, 384, N_MID, nq=768),
    _case("groups4-cos384", GROUPS, COS, 384, N_MID, nq=1024),
    _case("groups2-cos768", GROUPS, COS, 768, N_MID, nq=512),
    _case("groups3-cos768", GROUPS, COS, 768, N_MID, nq=768),
    _case("groups4-cos768", GROUPS, COS, 768, N_MID, nq=1024),
    _case("split-cos384", SPLIT, COS, 384, N_MID, tuning=(("batch_rega", 5),)),
    _case("split-cos768", SPLIT, COS, 768, N_MID, tuning=(("batch_rega", 5),)),
    _case("tiled-cos64", TILED, COS, 64, N_TILED),
    _case("tiled-dot192", TILED, DOT, 192, N_TILED),
    _case("tiled-l2-384", TILED, L2, 384, N_TILED),
    _case("slab-small-slabs", SLAB, COS, 384, N_SLAB, tuning=(("batch_onepass", 0), ("batch_slab_mb", 1))),
    _case("slab-default-slabs", SLAB, COS, 384, N_SLAB, tuning=(("batch_onepass", 0),)),
    _case("slab-below-floor", SLAB, COS, 384, N_FLOOR),
    _case("exact-cos384", EXACT, COS, 384, N_EXACT, tuning=(("batch_mode", 0),)),
    _case("exact-l2-100", EXACT, L2, 100, N_EXACT, tuning=(("batch_mode", 0),)),
    _case("handle-cos384", HANDLE, COS, 384, N_MID),
]
CERTIFIED_ROUTES = (POOL, FIXED, GROUPS, SPLIT, TILED, SLAB, HANDLE)
HANDLE_SHARDS = 3


def stores():
    """The distinct (metric, dims, rows) of the table, in its order."""
    seen = []
    for c in CASES:
        key = (c["metric"], c["dims"], c["n"])
        if key not in seen:
            seen.append(key)
    return seen


def fallback_cap(n):
    return -(-n // 1000)


# ---- the store ------------------------------------------------------------------------------------------------------------------------

def store_seed(metric, dims, n):
    return STORE_SEED + 1_000_003 * metric + 7_919 * dims + n


def partner(n):
    """partner(i) for every row; -1 for the lone last row of an odd store."""
    h = n // 2
    p = np.full(n, -1, dtype=np.int64)
    p[:h] = np.arange(h, 2 * h)
    p[h:2 * h] = np.arange(h)
    return p


def _unit(x):
    """Rows of an f32 array over their float64 norms (the result is f32: unit to a few 1e-8)."""
    return x / np.sqrt(np.einsum("ij,ij->i", x, x, dtype=np.float64))[:, None].astype(np.float32)


def _bf16(x):
    """helpers.bf16_rne for finite f32 values, in 32-bit integer arithmetic (no NaN / inf handling: the stores have none)."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    b = (b + np.uint32(0x7fff) + ((b >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xffff0000)
    return b.view(np.float32)


def twin_store(metric, dims, n, seed=None, block=32_768):
    """The store as f32 [n, dims], from numpy's generator (the GPU test draws its own on the device by the same recipe: what is
    proved here is about the construction, and (a) is asserted again on the rows the device drew)."""
    rng = np.random.default_rng(store_seed(metric, dims, n) if seed is None else seed)
    h = n // 2
    rows = np.empty((n, dims), dtype=np.float32)
    scale = DOT_SCALE if metric == DOT else 1.0
    for lo in range(0, h, block):
        hi = min(h, lo + block)
        base = _unit(rng.standard_normal((hi - lo, dims), dtype=np.float32))
        g = rng.standard_normal((hi - lo, dims), dtype=np.float32)
        g *= np.float32(SIGMA / math.sqrt(dims))
        g += base
        rows[lo:hi] = base
        rows[lo + h:hi + h] = _unit(g)
    if n % 2:
        rows[n - 1] = _unit(rng.standard_normal((1, dims), dtype=np.float32))[0]
    if scale != 1.0:
        rows *= np.float32(scale)
    return rows


# ---- the float64 model ----------------------------------------------------------------------------------------------------------------
DISTANCE_UNIT = {COS: 1.0, DOT: DOT_SCALE * DOT_SCALE, L2: 2.0}   # what a cosine distance of 1 between two rows is in the metric's distance


def _pair_scores(a, b, metric):
    """The metric's score (VectorMetric.score(fromDistance:)) of row pairs, in float64: cosine similarity; dot - 1 (the distance is
    1 - dot, the score its negative); minus the squared distance."""
    def dot(x, y):
        return np.einsum("ij,ij->i", x, y, dtype=np.float64)      # f32 operands, every product and sum in float64

    if metric == COS:
        return dot(a, b) / np.sqrt(dot(a, a) * dot(b, b))
    if metric == DOT:
        return dot(a, b) - 1.0
    e = a.astype(np.float64) - b.astype(np.float64)
    return -dot(e, e)


def expected(rows, metric, block=32_768):
    """(ids int64 [n, 2], scores float64 [n, 2]) of the sweep: [i, partner(i)], the self score and the pair's score. The lone row's
    second entry is (-1, nan): not checked."""
    n = rows.shape[0]
    p = partner(n)
    ids = np.stack([np.arange(n, dtype=np.int64), p], axis=1)
    scores = np.full((n, 2), np.nan)
    for lo in range(0, n, block):
        hi = min(n, lo + block)
        scores[lo:hi, 0] = _pair_scores(rows[lo:hi], rows[lo:hi], metric)
        has = p[lo:hi] >= 0
        idx = np.arange(lo, hi)[has]
        scores[idx, 1] = _pair_scores(rows[idx], rows[p[idx]], metric)
    return ids, scores


def pair_cosines(rows, block=32_768):
    """float64 cosine of every (row i, row i + H)."""
    h = rows.shape[0] // 2
    out = np.empty(h)
    for lo in range(0, h, block):
        hi = min(h, lo + block)
        out[lo:hi] = _pair_scores(rows[lo:hi], rows[lo + h:hi + h], COS)
    return out


def cap_bound(n, dims, t=CAP_T):
    """An upper bound on the expected number of ordered row pairs of n independent uniform unit vectors in R^dims with cosine >= t.
    For t >= 1 / sqrt(2) the cap {x: <x, e> >= t} lies in the ball of radius sqrt(1 - t^2) about t e, and so does the cone over it
    from the origin: its share of the unit ball, which is the cap's share of the sphere, is at most (1 - t^2)^(dims / 2)
    <= (1 - t^2)^((dims - 1) / 2). Every row of the twin store is uniform on the sphere and independent of every row but its twin."""
    assert t * t >= 0.5
    return float(n) * float(n) * (1.0 - t * t) ** ((dims - 1) / 2.0)


def stranger_best(rows, metric, block=2_048):
    """Per query of the sweep, the score of its best stranger — every row but the query's own and its twin — by a blocked f32
    matrix product over the whole store (an error of a few 1e-6 at these norms: the orderings asked of it are 0.05 and more apart).
    The score matrix is symmetric under all three metrics, so only the blocks on and above the diagonal are formed: a block's row
    maxima serve its own queries, its column maxima the queries behind it."""
    n = rows.shape[0]
    p = partner(n)
    norm2 = np.einsum("ij,ij->i", rows, rows, dtype=np.float64)
    x = (rows / np.sqrt(norm2)[:, None].astype(np.float32)) if metric == COS else rows
    x = np.ascontiguousarray(x, dtype=np.float32)
    n2 = norm2.astype(np.float32)
    best = np.full(n, -np.inf, dtype=np.float32)
    buf = np.empty((block, n), dtype=np.float32)
    for lo in range(0, n, block):
        hi = min(n, lo + block)
        s = buf[:hi - lo, :n - lo]
        np.matmul(x[lo:hi], x[lo:].T, out=s)                     # columns lo .. n - 1
        r = np.arange(hi - lo)
        s[r, r] = -np.inf
        has = p[lo:hi] >= lo                                     # (a twin in front of the block was masked in its own block's columns)
        s[r[has], p[lo:hi][has] - lo] = -np.inf
        if metric == L2:
            # - |a - b|^2 = 2 a.b - |a|^2 - |b|^2: a row's maximum needs the column term first, a column's the row term
            v_row = np.max(2.0 * s - n2[None, lo:], axis=1) - n2[lo:hi]
        else:
            v_row = np.max(s, axis=1)
        best[lo:hi] = np.maximum(best[lo:hi], v_row)
        if hi < n:                                               # the transposed part: queries hi .. n - 1 against the rows lo .. hi - 1
            t = s[:, hi - lo:]
            if metric == L2:
                v_col = np.max(2.0 * t - n2[lo:hi, None], axis=0) - n2[hi:]
            else:
                v_col = np.max(t, axis=0)
            best[hi:] = np.maximum(best[hi:], v_col)
    if metric == DOT:
        best -= np.float32(1.0)
    return best


def top3(rows, metric):
    """(int64 [n, 3], best stranger scores): the three best rows of every query of the sweep — self, twin and its best stranger,
    written n (a stranger, whichever: no answer of the model depends on which); the lone row: self, stranger, -1 — with the order
    self > twin > best stranger asserted on the scores of every query."""
    n = rows.shape[0]
    ids, scores = expected(rows, metric)
    best = stranger_best(rows, metric)
    paired = ids[:, 1] >= 0
    assert np.all(scores[paired, 0] > scores[paired, 1] + 1e-3) and np.all(scores[paired, 1] > best[paired] + 1e-3)
    assert np.all(scores[~paired, 0] > best[~paired] + 1e-3)
    return strangers_behind(ids), best


def strangers_behind(ids):
    """The three best rows of every query where no stranger outranks a twin: [i, partner(i), a stranger]; the lone row [i, a stranger, -1]."""
    n = ids.shape[0]
    out = np.stack([ids[:, 0], ids[:, 1], np.full(n, n)], axis=1)
    lone = ids[:, 1] < 0
    out[lone, 1] = n
    out[lone, 2] = -1
    return out


def drop_row(t3, r):
    """The checked answers of the sweep under a model filter that never sees row position r: every query's two best rows among its
    three best without r (one row less leaves the two best inside the three best), the lone row's second entry masked as in `expected`."""
    keep = t3 != r
    order = np.argsort(~keep, axis=1, kind="stable")          # kept entries first, in rank order
    out = np.take_along_axis(t3, order, axis=1)[:, :2].copy()
    lone = t3[:, 2] < 0
    out[lone, 1] = -1
    return out


def eps_worst(metric, dims, q_norm, v_max):
    """The certificate's eps (batch_prep_kernel) with the WORST-CASE error norms in place of the measured ones — the
    engine takes the smaller of the two. bf16 keeps 8 significant bits: rounding moves an element by at most 2^-8 relative, a product of
    two rounded elements by 2^-7 (1 + 2^-9); D products accumulated in f32 and the f32 normalisations add D 5.97e-8; relative to
    ||q|| max ||v|| (both 1 + 1e-6 under cosine, whose rows and queries are normalised first)."""
    qn, vn = (1.0 + 1e-6, 1.0 + 1e-6) if metric == COS else (float(q_norm), float(v_max))
    u = 0.0078125 * (1.0 + 1.0 / 512.0) + dims * 5.97e-8 + 1e-6
    dot_err = u * qn * vn * 1.001
    if metric == COS:
        return dot_err + 3e-6
    if metric == DOT:
        return dot_err + 1e-6 * (1.0 + qn * vn)
    return 2.0 * dot_err + 4e-6 * (1.0 + float(q_norm) ** 2 + float(v_max) ** 2)


def certificate_margins(rows, metric, sample, block=65_536):
    """For the queries `sample` (paired rows): a_max - eps - d2, where a_max is the KP-th smallest approximate distance of the query
    over the whole store (bf16 roundings of both sides, normalised first under cosine, products summed in f32 — the f32 sum's own
    error, at most dims 2^-23 of the product of the norms, is taken off as well), eps = eps_worst and d2 the exact float64 distance
    of the query's twin, its second neighbour. Positive = the first finish certifies the query even at the worst-case eps."""
    n, dims = rows.shape
    p = partner(n)
    assert np.all(p[sample] >= 0)
    norms = np.sqrt(np.einsum("ij,ij->i", rows, rows, dtype=np.float64))
    unit = metric == COS

    def mirror(x, nx):
        return _bf16((x / nx[:, None].astype(np.float32)) if unit else x)

    qb = mirror(rows[sample], norms[sample])
    approx = np.empty((len(sample), n), dtype=np.float32)
    for lo in range(0, n, block):
        hi = min(n, lo + block)
        approx[:, lo:hi] = qb @ mirror(rows[lo:hi], norms[lo:hi]).T
    approx *= np.float32(-2.0 if metric == L2 else -1.0)      # in place, f32: the distance less the terms added below
    if metric == L2:
        approx += (norms ** 2).astype(np.float32)[None, :]
    approx.partition(KP - 1, axis=1)
    a_max = approx[:, KP - 1].astype(np.float64) + (norms[sample] ** 2 if metric == L2 else 1.0)
    pair = _pair_scores(rows[sample], rows[p[sample]], metric)
    second = 1.0 - pair if metric == COS else -pair
    v_max = float(np.max(norms))
    eps = np.array([eps_worst(metric, dims, norms[i], v_max) for i in sample])
    f32_sum = (dims + 4) * 2.0 ** -23 * (1.0 if unit else norms[sample] * v_max) * (2.0 if metric == L2 else 1.0)
    return a_max - eps - f32_sum - second


def margin_sample(n, seed=1):
    """At least MARGIN_SAMPLE paired rows: the first and the last of each half, and seeded random ones."""
    h = n // 2
    rng = np.random.default_rng(seed)
    pick = np.concatenate([[0, h - 1, h, 2 * h - 1], rng.choice(2 * h, MARGIN_SAMPLE, replace=False)])
    return np.unique(pick)


# ---- the rows whose batched answer is compared bit for bit with searchArrays -----------------------------------------------------------

def bit_sample(metric, dims, n, nq, shard_bases=(), count=32, seed=2):
    """`count` rows of the sweep: rows 0 and n - 1; the first and last row of the last fixed tile and of the first pool tile where the
    filtering GEMM has a pool; the first and last row of the ragged last tile; the rows on each side of every shard boundary; seeded
    random rows."""
    tr = tile_rows(metric, dims)
    pick = [0, n - 1, (n - 1) // tr * tr]
    pool = pool_first_row(metric, dims, n, nq)
    if pool is not None:
        pick += [pool - tr, pool - 1, pool, pool + tr - 1]
    for b in shard_bases:
        if 0 < b < n:
            pick += [b - 1, b]
    pick = list(dict.fromkeys(int(x) for x in pick))
    rng = np.random.default_rng(seed + n + dims)
    for r in rng.permutation(n):
        if len(pick) >= count:
            break
        if int(r) not in pick:
            pick.append(int(r))
    return np.array(sorted(pick[:count]), dtype=np.int64)
