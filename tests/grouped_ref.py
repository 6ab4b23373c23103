"""A numpy restatement of wax_hip_search_grouped's contract (include/wax_hip.h; PhotoRAGOrchestrator.swift:264-317,
VideoRAGOrchestrator.swift:273-417) from what the device sees: every row's key, its parent, its frame id and the row bitmap.

A key is the project's make_key(distance, row) (wax_amd/csrc/common.h): the distance's ordered bits in the high word, the row in the
low one, so int64 order is (distance ascending, row ascending). A row whose distance is not finite takes no part. A row's root is
its parent, or its own frame id where the parent is NO_PARENT. Groups are ordered by (distance bits ascending, root id ascending as
unsigned); inside a group the members by key ascending.

The case tables at the end are shared by the CPU tests, which prove them to be what they claim, and the GPU tests, which run them."""
from collections import namedtuple

import numpy as np

NO_PARENT = np.uint64((1 << 64) - 1)
KEY_PAD = np.int64((1 << 63) - 1)
ID_PAD = np.uint64((1 << 64) - 1)
MAX_LIMIT = 1024
MAX_MEMBERS = 8


def order_bits(dist):
    """common.h order_bits: float32 -> int32 whose signed order is the float order."""
    b = np.ascontiguousarray(dist, dtype=np.float32).view(np.int32)
    return b ^ ((b >> 31) & np.int32(0x7fffffff))


def unorder_bits(o):
    o = np.ascontiguousarray(o, dtype=np.int32)
    return (o ^ ((o >> 31) & np.int32(0x7fffffff))).view(np.float32)


def make_keys(dist, rows=None):
    """int64 key of every row; KEY_PAD where the distance is not finite (such a row takes no part)."""
    dist = np.ascontiguousarray(dist, dtype=np.float32).reshape(-1)
    rows = np.arange(dist.size, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    keys = (order_bits(dist).astype(np.int64) << 32) | rows
    return np.where(np.isfinite(dist), keys, KEY_PAD)


def key_bits(keys):
    return (np.asarray(keys, dtype=np.int64) >> 32).astype(np.int32)


def key_rows(keys):
    return (np.asarray(keys, dtype=np.int64) & 0xffffffff).astype(np.int64)


def roots_of(parents, frame_ids):
    frame_ids = np.asarray(frame_ids, dtype=np.uint64)
    if parents is None:
        return frame_ids.copy()
    parents = np.asarray(parents, dtype=np.uint64)
    return np.where(parents != NO_PARENT, parents, frame_ids)


def bitmap_of(passing):
    """bool per row -> the uint32 words the device reads."""
    passing = np.asarray(passing, dtype=bool)
    words = np.zeros((passing.size + 31) // 32, dtype=np.uint32)
    r = np.nonzero(passing)[0]
    np.bitwise_or.at(words, r >> 5, (np.uint32(1) << (r & 31).astype(np.uint32)))
    return words


Answer = namedtuple("Answer", "roots bits member_keys counts")


def grouped_model(keys, parents, frame_ids, passing, limit, per_group):
    """(root ids [g], distance bits [g] int32, member keys [g, per_group] padded with KEY_PAD, member counts [g])."""
    keys = np.asarray(keys, dtype=np.int64)
    per_group = max(1, int(per_group))
    roots = roots_of(parents, frame_ids)
    part = keys != KEY_PAD
    if passing is not None:
        part &= np.asarray(passing, dtype=bool)
    groups = {}
    for r in np.nonzero(part)[0].tolist():
        groups.setdefault(int(roots[r]), []).append(int(keys[r]))
    ranked = sorted(((min(ks) >> 32, root) for root, ks in groups.items()))   # Python ints: the root compares as unsigned
    ranked = ranked[:max(0, int(limit))]
    g = len(ranked)
    out_roots = np.array([root for _, root in ranked], dtype=np.uint64)
    out_bits = np.array([b for b, _ in ranked], dtype=np.int64).astype(np.int32)
    members = np.full((g, per_group), KEY_PAD, dtype=np.int64)
    counts = np.zeros(g, dtype=np.uint32)
    for i, (_, root) in enumerate(ranked):
        ks = sorted(groups[root])[:per_group]
        members[i, :len(ks)] = ks
        counts[i] = len(ks)
    return Answer(out_roots, out_bits, members, counts)


def score_of(bits, metric="cosine"):
    """VectorMetric.score(fromDistance:) in float32, as the library applies it."""
    d = unorder_bits(bits)
    return (np.float32(1.0) - d) if metric == "cosine" else -d


def apply_cut(ans, min_score, metric="cosine"):
    """Rule 7: groups below the cut are dropped, as are members below it. `score < cut` drops."""
    g_scores = score_of(ans.bits, metric)
    keep = ~(g_scores < np.float32(min_score))
    members = ans.member_keys[keep].copy()
    m_scores = score_of(key_bits(members), metric)
    below = (members != KEY_PAD) & (m_scores < np.float32(min_score))
    members[below] = KEY_PAD
    counts = (members != KEY_PAD).sum(axis=1).astype(np.uint32)
    return Answer(ans.roots[keep], ans.bits[keep], members, counts)


def collapse_prefix(keys, parents, frame_ids, passing, top_k, limit):
    """What a caller does today (VideoRAGOrchestrator.swift:252, 273-417): rank the top_k best ROWS, collapse them by root,
    order the roots by (best score, root id), keep `limit`. Returns the root ids."""
    keys = np.asarray(keys, dtype=np.int64)
    roots = roots_of(parents, frame_ids)
    part = keys != KEY_PAD
    if passing is not None:
        part &= np.asarray(passing, dtype=bool)
    rows = np.nonzero(part)[0]
    rows = rows[np.argsort(keys[rows], kind="stable")][:top_k]
    best = {}
    for r in rows.tolist():
        root = int(roots[r])
        best[root] = min(best.get(root, int(keys[r]) >> 32), int(keys[r]) >> 32)
    ranked = sorted((b, root) for root, b in best.items())[:limit]
    return np.array([root for _, root in ranked], dtype=np.uint64)


def merge_shards(answers, limit):
    """The handle's merge (per_group 1): the smaller distance per root — the lower shard on equal bits — then (distance, root id)."""
    best = {}
    for a in answers:
        for root, b, mk in zip(a.roots.tolist(), a.bits.tolist(), a.member_keys[:, 0].tolist()):
            if root not in best or b < best[root][0]:
                best[root] = (b, mk)
    ranked = sorted((b, root) for root, (b, _) in best.items())[:limit]
    return (np.array([root for _, root in ranked], dtype=np.uint64), np.array([b for b, _ in ranked], dtype=np.int64).astype(np.int32))


# ---- the probe's case table: made-up distances, bit for bit -----------------------------------------------------------------

GRIDS = (1, 2, 3)
ProbeCase = namedtuple("ProbeCase", "name dist parents frame_ids passing limit per_group")


def slots_of(parents, frame_ids):
    """A dense numbering of the roots in order of first appearance: (slot per row uint32, root per slot uint64)."""
    roots = roots_of(parents, frame_ids)
    uniq, first, inv = np.unique(roots, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty_like(order)
    rank[order] = np.arange(order.size)
    return rank[inv].astype(np.uint32), uniq[order]


def _probe_cases():
    rng = np.random.default_rng(32)
    cases = []
    n = 20000
    ids = rng.permutation(n).astype(np.uint64) + np.uint64(1000)
    # blocks of equal bits that straddle the 256-row tiles the workgroups stride by: rows 200 .. 327, 480 .. 560 etc. share a distance
    dist = rng.random(n, dtype=np.float32) + np.float32(0.25)
    for lo, hi, v in ((200, 328, 0.125), (480, 560, 0.125), (1000, 1300, 0.0625), (19900, 20000, 0.0625), (5000, 5003, 0.03125)):
        dist[lo:hi] = np.float32(v)
    parents = np.full(n, NO_PARENT, dtype=np.uint64)
    grouped = rng.random(n) < 0.8
    parents[grouped] = rng.integers(1 << 40, (1 << 40) + 700, size=int(grouped.sum())).astype(np.uint64)   # roots the store does not hold
    # the best rows: three of one root with equal bits, then forty roots that share the two 0.0625 blocks at both ends of the store
    parents[5000:5003] = np.uint64(1 << 41)
    parents[1000:1300] = np.uint64(1 << 40) + rng.integers(0, 40, size=300).astype(np.uint64)
    parents[19900:20000] = np.uint64(1 << 40) + rng.integers(0, 40, size=100).astype(np.uint64)
    cases.append(ProbeCase("tied-blocks-l12-p3", dist, parents, ids, None, 12, 3))
    cases.append(ProbeCase("tied-blocks-l1024-p8", dist, parents, ids, None, 1024, 8))
    cases.append(ProbeCase("tied-blocks-l1-p1", dist, parents, ids, None, 1, 1))
    passing = rng.random(n) < 0.5
    passing[200:328] = False
    cases.append(ProbeCase("tied-blocks-masked-l40-p4", dist, parents, ids, passing, 40, 4))
    cases.append(ProbeCase("singletons-l64-p2", dist, None, ids, None, 64, 2))
    # every distance equal: the order is the root ids' alone, the members' the rows' alone
    flat = np.full(4097, np.float32(0.5), dtype=np.float32)
    fids = rng.permutation(4097).astype(np.uint64)
    fpar = (np.uint64(1 << 63) + (np.arange(4097, dtype=np.uint64)[::-1] // np.uint64(5))).astype(np.uint64)   # root ids above 2^63, descending with the row
    cases.append(ProbeCase("all-equal-unsigned-roots-l30-p8", flat, fpar, fids, None, 30, 8))
    # negative, zero, -0 and non-finite distances
    odd = rng.standard_normal(257).astype(np.float32)
    odd[::7] = np.float32(0.0)
    odd[3::7] = np.float32(-0.0)
    odd[5::31] = np.float32(np.inf)
    odd[6::31] = np.float32(-np.inf)
    odd[8::31] = np.float32(np.nan)
    opar = (np.arange(257, dtype=np.uint64) % np.uint64(19)) + np.uint64(7)
    cases.append(ProbeCase("signs-and-nonfinite-l19-p8", odd, opar, np.arange(257, dtype=np.uint64) + np.uint64(500), None, 19, 8))
    cases.append(ProbeCase("nothing-passes", odd, opar, np.arange(257, dtype=np.uint64) + np.uint64(500), np.zeros(257, dtype=bool), 5, 2))
    return tuple(cases)


PROBE_CASES = _probe_cases()


def probe_expected(case):
    keys = make_keys(case.dist)
    return grouped_model(keys, case.parents, case.frame_ids, case.passing, case.limit, case.per_group)


# ---- corpora of the engine tests: (parents per row, frame ids per row) for a store of n rows --------------------------------

def partition(kind, n, seed=0):
    """Parents and frame ids of an n-row store. `none`: no parent set (parents None), frame ids ascending. `one`: every row one
    root the store does not hold. `scattered`: roots of 1 to 40 rows scattered over the store, frame ids a permutation of the rows,
    some rows their own root, some roots rows of the store. `foreign`: every root an id the store does not hold."""
    rng = np.random.default_rng(1000 + seed)
    if kind == "none":
        return None, np.arange(n, dtype=np.uint64) + np.uint64(100)
    if kind == "one":
        return np.full(n, np.uint64(77_000_000), dtype=np.uint64), rng.permutation(n).astype(np.uint64)
    fids = rng.permutation(n).astype(np.uint64)
    parents = np.full(n, NO_PARENT, dtype=np.uint64)
    order = rng.permutation(n)
    at = 0
    while at < n:
        size = int(rng.integers(1, 41))
        rows = order[at:at + size]
        at += size
        if kind == "foreign":
            parents[rows] = np.uint64(1 << 50) + np.uint64(at)
        elif size > 1:
            head = rows[0]
            parents[rows[1:]] = fids[head]                       # the root is a row of the store, and is its own root
            if rng.random() < 0.3:
                parents[head] = fids[head]                       # ... said explicitly
    return parents, fids
