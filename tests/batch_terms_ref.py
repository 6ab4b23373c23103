"""A numpy restatement of term_mask_multi_kernel (wax_amd/csrc/terms.hip) and made-up columns for its probe.

The kernel decides up to 32 required-term sets per row in one walk of the row's values: the sorted union U of the sets' terms, a
membership word per union term (bit s = "set s requires it"), five bit-sliced counter words per row (bit s of c4..c0 = how many terms of
set s the row holds) and five bit planes of the sets' sizes. multi_model() does exactly that arithmetic; containment() is the
specification it is held to: a row passes set s when the row's values contain every term of set s."""
import numpy as np

import terms_ref as ref

MAX_SETS = 32           # TERM_MULTI_MAX_SETS
MAX_UNION = 512         # TERM_MULTI_MAX_UNION


def plan(sets):
    """(U ascending, memb[u] with bit s = set s requires U[u], N0..N4 with bit s of N_p = bit p of |set s|, live sets mask)."""
    sets = [sorted(set(int(t) for t in s)) for s in sets]
    assert 1 <= len(sets) <= MAX_SETS and all(1 <= len(s) <= ref.MAX_REQUIRED for s in sets)
    uni = np.array(sorted(set(t for s in sets for t in s)), dtype=np.uint32)
    memb = np.zeros(len(uni), dtype=np.uint32)
    nbits = np.zeros(5, dtype=np.uint32)
    for i, s in enumerate(sets):
        memb[np.searchsorted(uni, np.array(s, dtype=np.uint32))] |= np.uint32(1 << i)
        for p in range(5):
            nbits[p] |= np.uint32(((len(s) >> p) & 1) << i)
    return uni, memb, nbits, np.uint32((1 << len(sets)) - 1)


def pass_words(off, val, sets):
    """The kernel's pass word of every row (bit s = the row passes set s), by the kernel's arithmetic."""
    uni, memb, nbits, live = plan(sets)
    off = np.asarray(off, dtype=np.int64)
    val = np.asarray(val, dtype=np.uint32)
    n = len(off) - 1
    lens = np.diff(off)
    c = np.zeros((5, n), dtype=np.uint32)
    for j in range(int(lens.max(initial=0))):
        rows = np.nonzero(lens > j)[0]
        x = val[off[rows] + j]
        inside = (x >= uni[0]) & (x <= uni[-1])                    # the range test against U's ends
        idx = np.minimum(np.searchsorted(uni, x), len(uni) - 1)    # the bisection
        carry = np.where(inside & (uni[idx] == x), memb[idx], 0).astype(np.uint32)
        for p in range(5):
            t = c[p, rows] & carry
            c[p, rows] ^= carry
            carry = t
        assert not carry.any()                                     # a counter never exceeds |set s| <= 16 < 32
    diff = np.zeros(n, dtype=np.uint32)
    for p in range(5):
        diff |= c[p] ^ nbits[p]
    return ~diff & live


def multi_model(off, val, sets):
    """(bitmaps uint32 [S, words], counts uint32 [S]): what term_mask_multi_kernel writes."""
    w = pass_words(off, val, sets)
    bits = [((w >> np.uint32(s)) & 1).astype(bool) for s in range(len(sets))]
    return np.stack([ref.bitmap_of(b) for b in bits]), np.array([int(b.sum()) for b in bits], dtype=np.uint32)


def containment(off, val, sets):
    """The same two arrays from the specification: row r passes set s when values[off[r] .. off[r + 1]) hold every term of set s."""
    bits = [ref.pass_csr(np.asarray(off), np.asarray(val), s) for s in sets]
    return np.stack([ref.bitmap_of(b) for b in bits]), np.array([int(b.sum()) for b in bits], dtype=np.uint32)


# ---- made-up sets and columns --------------------------------------------------------------------------------------------------
# Set terms lie in [LO, HI); a row's other values lie below LO, above HI, or between them on values no set uses (odd ones).
LO, HI = 10_000, 30_000
SIZES = (1, 2, 15, 16)


def make_sets(family, n_sets, rng):
    """family "disjoint16": n_sets sets of 16 terms, pairwise disjoint — the union of 32 of them is exactly 512 terms.
    family "shared": sizes cycle through 1, 2, 15, 16 counting the ONE term every set requires; where there are two or more sets,
    set 1 is a subset of set 0. Set terms are even numbers."""
    pool = (LO + 2 * rng.permutation((HI - LO) // 2)).astype(np.int64)
    if family == "disjoint16":
        return [sorted(int(t) for t in pool[16 * s:16 * s + 16]) for s in range(n_sets)]
    common, pool = int(pool[0]), pool[1:]
    sets, at = [], 0
    for s in range(n_sets):
        size = SIZES[(s + 3) % 4]                                   # 16, 1, 2, 15, 16, ...
        own = [int(t) for t in pool[at:at + size - 1]]
        at += size - 1
        sets.append(sorted([common] + own))
    if n_sets >= 2:
        sets[1] = sorted(sets[0][:8] if common in sets[0][:8] else [common] + sets[0][:7])
    return sets


def noise(rng, k):
    """k distinct values no set holds: below LO, above HI, and odd ones between."""
    below = rng.integers(0, LO, size=k)
    above = rng.integers(HI, 2**32 - 1, size=k)
    between = LO + 1 + 2 * rng.integers(0, (HI - LO) // 2 - 1, size=k)
    pick = rng.integers(0, 3, size=k)
    return np.where(pick == 0, below, np.where(pick == 1, above, between))


KINDS = ("empty", "one", "full64", "full", "minus_one", "spread", "noise", "everything")


def make_rows(sets, n, rng):
    """n rows, each of one of KINDS (returned beside them): no value; ONE value (of the union, or noise); all of a set and noise up to 64
    values; all of a set and a little noise; all but one term of a set; |set s| terms of the union taken from sets s and t, not all of
    either; noise only; as many whole sets as fit 64 values."""
    kinds = rng.integers(0, len(KINDS), size=n)
    union = sorted(set(t for s in sets for t in s))
    rows = []
    for r in range(n):
        kind = KINDS[kinds[r]]
        s = sets[int(rng.integers(0, len(sets)))]
        if kind == "empty":
            v = []
        elif kind == "one":
            v = [union[int(rng.integers(0, len(union)))]] if rng.random() < 0.7 else list(noise(rng, 1))
        elif kind == "full64":
            v = list(s) + list(noise(rng, 200))
        elif kind == "full":
            v = list(s) + list(noise(rng, int(rng.integers(0, 6))))
        elif kind == "minus_one":
            v = list(s)
            del v[int(rng.integers(0, len(v)))]
            v += list(noise(rng, int(rng.integers(0, 4))))
        elif kind == "spread":
            t = sets[int(rng.integers(0, len(sets)))]
            half = len(s) // 2
            v = list(s[:half]) + [x for x in t if x not in s][:len(s) - half]
        elif kind == "noise":
            v = list(noise(rng, int(rng.integers(1, 30))))
        else:
            v = []
            for t in rng.permutation(len(sets)):
                if len(set(v) | set(sets[int(t)])) <= ref.MAX_PER_ROW:
                    v = sorted(set(v) | set(sets[int(t)]))
        v = np.unique(np.asarray(v, dtype=np.int64))
        if len(v) > ref.MAX_PER_ROW:                                # keep the set's own terms (the even ones in [LO, HI)), drop noise
            own = v[(v >= LO) & (v < HI) & (v % 2 == 0)]
            rest = v[~np.isin(v, own)]
            v = np.sort(np.concatenate([own, rest[:ref.MAX_PER_ROW - len(own)]]))
        rows.append(tuple(int(x) for x in v))
    return rows, [KINDS[k] for k in kinds]
