"""What test_selection_edges_gpu.py relies on, proven on the CPU for every store, column, k and row_base it uses (selection_ref.py):
the model equals the f64 oracle; each construction has the property that lets its GPU case fail (a tie group that straddles rank k or
ends on it, the radix pass that decides, row numbers that cross byte boundaries, the non-finite counts); the restated radix selection
equals the model; and each of four lines of select_hist_kernel (its `n % 4` tail, the `all_needed` branch, the
`(u >> (shift + 8)) == prefix` match, the four-in-flight loop's row index `4 * j4`), reverted in that restatement, changes the answer
of a named GPU case."""
import numpy as np
import pytest

import oracle
import selection_ref as R


@pytest.fixture(scope="module")
def stores():
    return {name: R.build_store(name) for name in R.STORE_NAMES}


def cases(stores, names=R.STORE_NAMES):
    for name in names:
        metric, rows, cols = stores[name]
        for cname, (q, col, extra) in cols.items():
            yield name, metric, rows, cname, q, col, R.ks_of(cname, col, extra)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the model against the oracle ------------------------------------------------------------------------------------------------

def test_model_equals_the_f64_oracle(stores):
    """ids and scores bit for bit, every (store, column, k). Every distance here is one correctly rounded f32 operation on exact
    inputs, which the oracle's f64 arithmetic followed by one rounding to f32 reproduces — `wide` included (1 - 2^-149 rounds to 1
    in f64 and in f32 alike), so no pair is left out for the oracle's wider arithmetic. One pair is checked differently: the
    non-finite store at k = n. With NaN distances among the rows its heap is seeded with, the oracle's comparator (wax_oracle.c:248:
    `a->d < b->d || (a->d == b->d && ...)`) is not a strict weak order, so there the oracle's own selection (wax_oracle_topk_total)
    is run on the model's canonical distances (NaN -> +inf, as finish_distance writes them) instead of on its own NaN."""
    for name, metric, rows, cname, q, col, ks in cases(stores):
        for k in ks:
            ids, scores = col.answer(k)
            ctx = f"{name} {cname} k={k}"
            if cname == "non-finite" and k >= R.NON_FINITE_NAN_ROWS[0]:
                idx, dd = oracle.topk_heap(col.d, R.clamp_topk(k), total=True)
                keep = np.isfinite(dd)
                assert np.array_equal(ids, col.ids[idx[keep]]) and np.array_equal(bits(scores), bits(-dd[keep])), ctx
                continue
            e_ids, e_scores, _, _ = oracle.search(metric, rows, col.ids, q, k)
            assert np.array_equal(ids, e_ids), ctx
            assert np.array_equal(bits(scores), bits(e_scores)), ctx
        for rb in R.row_bases_for(col.n):                                # global rows ascend with local rows: one answer for every row_base
            assert np.array_equal(col.order(rb), col.order(0)), (name, cname, rb)


def test_ladder_distances_round_trip():
    """f32(1) - x is the d each ladder was meant to hold, bit for bit — and a d that 1 - (1 - d) does not give back is refused."""
    for n in (R.N_BIG,) + R.SMALL_NS:
        intended = {}
        cols = R.dot_columns(n, intended=intended)
        assert set(intended) == set(R.LADDERS)
        for name in R.LADDERS:
            R.check_round_trip(cols[name], intended[name], f"{name} at {n} rows")
    d = np.array([0.75, 2.0 ** -30], dtype=np.float32)              # 1 - 2^-30 rounds to 1: the distance comes back as 0
    with pytest.raises(AssertionError):
        R.check_round_trip((R.ONE - d).astype(np.float32), d, "a d that does not survive")


# ---- the restated radix selection -------------------------------------------------------------------------------------------------

def test_restated_radix_selection_equals_the_model(stores):
    """Every (store, column, k, row_base): the eight passes, the compaction and the sort as kernels.hip writes them select the
    model's keys, and the pass that decides is the one the sorted keys imply (Column.deciding_pass)."""
    for name, metric, rows, cname, q, col, ks in cases(stores):
        for rb in R.row_bases_for(col.n):
            for k in ks:
                kk = min(R.clamp_topk(k), col.n)
                keys, decided, _ = R.radix_select(col.d, rb, kk)
                ctx = f"{name} {cname} k={k} row_base={rb:#x}"
                assert keys is not None and np.array_equal(keys, R.model_keys(col, k, rb)), ctx
                assert decided == col.deciding_pass(k, rb), ctx


def test_loops_the_grids_drive():
    """select_grid 4 on 70 001 rows: a stride of 1 024 float4s, so all three loops of select_hist_kernel, both of
    select_compact_kernel and the one-row tail run; select_grid 1: the four-deep loop 17 times per thread; the default grid (274
    workgroups) only the single-trip loop. The default-grid case: the smallest row count whose first thread takes the four-deep loop
    at 2 048 workgroups (one thread, 16 rows), two-deep for every other thread, a tail of 3."""
    n = R.N_BIG
    assert n % 4 == 1 and n >= 256 * 193 and n > 65536
    assert set(np.unique(R.hist_loops(n, R.select_grid_for(n, 4))[0])) == {1, 2, 4}
    assert set(np.unique(R.compact_loops(n, 4))) == {1, 2}
    assert set(np.unique(R.hist_loops(n, 1)[0])) == {1, 4}
    assert R.select_grid_for(n) == 274 and set(np.unique(R.hist_loops(n, 274)[0])) == {1}
    grid, four, two, tail = R.big_default_grid_loops()
    assert (grid, four, tail) == (2048, 16, 3) and two > 4_000_000
    smaller = R.BIG_N - 4                                             # one float4 less: nobody takes the four-deep loop
    assert not np.any(R.hist_loops(smaller, 2048)[0] == 4)


# ---- what each construction must have -------------------------------------------------------------------------------------------

def test_flat_and_straddle_groups(stores):
    metric, rows, cols = stores["dot-70001x64"]
    flat = cols["flat"][1]
    for k in R.ks_of("flat", flat):
        assert flat.tie_group(k) == (1, flat.n)
        assert np.array_equal(flat.taken(k), np.arange(min(k, flat.n)))          # rows 0 .. k - 1
        for rb in R.ROW_BASES:
            assert flat.deciding_pass(k, rb) >= 4                                   # decided purely in the row digits
    for g in (200, 300, 66000):
        col = cols[f"straddle-{g}"][1]
        low = np.nonzero(col.d == np.float32(0.5))[0]
        assert len(low) == g and low[-1] == col.n - 1 and np.all(col.d[np.setdiff1d(np.arange(col.n), low)] == np.float32(0.75))
        if g > R.MAX_RESULTS:                                                        # every k the clamp lets through is inside the group
            for k in R.ks_of(f"straddle-{g}", col):
                assert col.tie_group(k) == (1, g) and all(col.deciding_pass(k, rb) >= 4 for rb in R.ROW_BASES)
            continue
        assert col.tie_group(g - 1) == (1, g)                                        # straddles
        assert col.tie_group(g) == (1, g)                                            # ends exactly on k
        assert col.tie_group(g + 1) == (g + 1, col.n)                                # the first of the upper group
        assert col.taken(g + 1)[-1] == np.nonzero(col.d == np.float32(0.75))[0][0]  # ... its lowest row
        for rb in R.ROW_BASES:
            keys, decided, by_all = R.radix_select(col.d, rb, g)
            assert decided == 1 and by_all                                           # `all_needed` in a distance digit (0.5 | 0.75: the second byte)
            assert R.radix_select(col.d, rb, g - 1)[1] >= 4 and R.radix_select(col.d, rb, g + 1)[1] >= 4


def test_ladders_decide_in_the_claimed_pass(stores):
    """ladder-low-byte: the whole column shares the three leading key bytes (passes 0-2: every wave in one bin, the fast path of
    count_one), the fourth separates the values (its mixed branch). ladder-carry / ladder-exponent: two values of the second byte
    (..3F FF FF | ..40 00 00, ..7F FF FF | ..80 00 00), one bin again in the third among the keys that still match, and the fourth
    decides. Multiplicities leave ranks inside a value's rows (the row digits go on) and on their end (`all_needed` at pass 3)."""
    metric, rows, cols = stores["dot-70001x64"]
    for name, lead in (("ladder-low-byte", 1), ("ladder-carry", 2), ("ladder-exponent", 2)):
        col = cols[name][1]
        u = R.ukeys(col.d, 0)
        assert len(np.unique(u >> np.uint64(56))) == 1
        assert len(np.unique(u >> np.uint64(48))) == lead and len(np.unique(u >> np.uint64(40))) == lead
        assert len(np.unique(u >> np.uint64(32))) > 250
        passes = {k: col.deciding_pass(k) for k in R.KS}
        assert min(passes.values()) >= 3
        groups = [col.tie_group(k) for k in R.KS]
        assert sum(1 for (lo, hi), k in zip(groups, R.KS) if hi > k) >= 5                # straddled ranks
        first, last = col.tie_group(1000)
        assert R.radix_select(col.d, 0, last)[1:] == (3, True)                           # a rank on a value's last row: pass 3, all needed
    col = cols["ladder-carry"][1]
    top = np.sort(col.d)[:R.MAX_RESULTS]
    assert top[0] < np.float32(0.75) <= top[-1]                                          # the carry lies inside the ranks queried
    col = cols["ladder-exponent"][1]
    top = np.sort(col.d)[:R.MAX_RESULTS]
    assert top[0] < np.float32(1.0) <= top[-1]


def test_around_zero_and_wide_cover_the_sign(stores):
    """Negative distances (q.v > 1) come first and, as unsigned keys, in reversed bit order: -2^-20 before -2^-23 before 0."""
    metric, rows, cols = stores["dot-70001x64"]
    col = cols["around-zero"][1]
    d = col.d[col.taken(10000)]
    assert d[0] == np.float32(-2.0 ** -20) and np.all(np.diff(d) >= 0)
    neg, zero = int(np.sum(d < 0)), int(np.sum(d == 0))
    assert neg > 800 and zero > 100 and np.sum(d > 0) > 5000
    assert not np.any(np.signbit(col.d[col.d == 0]))                                     # 1 - 1 = +0
    u = R.ukeys(col.d, 0)
    assert np.all((u[col.d < 0] >> np.uint64(63)) == 0) and np.all((u[col.d >= 0] >> np.uint64(63)) == 1)
    straddled = [k for k in R.KS if col.tie_group(k)[1] > k]
    assert len(straddled) >= 4
    wide = cols["wide"][1]
    assert np.all(np.isfinite(wide.d)) and wide.d.min() == np.float32(1.0) - np.float32(2.0 ** 127) and wide.d.max() == np.float32(2.0 ** 127)
    assert np.sum(wide.d == 1.0) > 1000                                                  # every |x| < 2^-25, the subnormals and +-0: one tie group
    assert np.all(np.isfinite(rows))                                                     # 0 * junk is an exact zero


def test_row_numbers_cross_byte_boundaries(stores):
    """row_base 0: 70 001 rows cross 2^16 (the third row byte takes two values). 0x00FFFF00: the rows cross 2^24 (at local row 256)
    and 2^16; 0xFFFE0000: they cross 0xFFFF0000 with the two top bytes all ones or nearly (the carry bytes of a large row_base),
    and row_base + n stays below 2^32. On `flat` and `straddle-66000` the rows taken at the larger k lie on both sides."""
    n = R.N_BIG
    assert R.row_bases_for(n) == list(R.ROW_BASES) and R.ROW_BASES[2] + n < 2 ** 32
    for rb, top, third in ((0, 1, 2), (0x00FFFF00, 2, 3), (0xFFFE0000, 1, 2)):
        g = rb + np.arange(n, dtype=np.uint64)
        assert len(np.unique(g >> np.uint64(24))) == top and len(np.unique(g >> np.uint64(16))) == third
    metric, rows, cols = stores["dot-70001x64"]
    for cname in ("flat", "straddle-66000"):
        col = cols[cname][1]
        g = 0x00FFFF00 + col.taken(4096).astype(np.uint64)
        assert len(np.unique(g >> np.uint64(24))) == 2 and len(np.unique(g >> np.uint64(16))) >= 2
        assert len(np.unique((0xFFFE0000 + np.arange(n, dtype=np.uint64)[col.d == col.d[col.taken(1)[0]]]) >> np.uint64(16))) == 2
    for small in R.SMALL_NS + (R.NON_FINITE_N,):
        assert R.row_bases_for(small) == list(R.ROW_BASES)


def test_non_finite_counts(stores):
    metric, rows, cols = stores["non-finite-1027x64"]
    q, col, extra = cols["non-finite"]
    n = col.n
    assert n == R.NON_FINITE_N and extra == (n,)
    assert np.sum(col.x == np.inf) == 7 and np.sum(col.x == -np.inf) == 5 and np.sum(np.isnan(col.x)) == 5
    assert np.sum(col.d == -np.inf) == 7 and np.sum(col.d == np.inf) == 10 and not np.any(np.isnan(col.d))
    assert np.all(np.isfinite(rows[:, 1:])) and not np.isnan(col.x[0])
    for k in R.ks_of("non-finite", col, extra):
        want = n - 17 if k >= n else (max(0, k - 7) if k <= 1000 else 1010)
        assert len(col.answer(k)[0]) == want, k
        assert np.all(col.d[col.taken(k)[:min(k, 7)]] == -np.inf)                        # they win their slots, then are dropped


def test_l2_and_cosine_groups(stores):
    for name in ("l2-70001x64", "l2-1023x64"):
        q, col, ranks = stores[name][2]["l2"]
        z = R.L2_ZEROS + R.L2_UNDERFLOW
        assert np.sum(col.d == 0) == z and np.sum(col.x == 0) == R.L2_ZEROS            # 2^-160 underflows: one group with the true zeros
        sub = (col.d > 0) & (col.d < np.float32(2.0 ** -126))
        assert np.sum(sub) == 7 * R.L2_SUBNORMAL_EACH and len(np.unique(col.d[sub])) == 7
        assert np.sum(np.isinf(col.d)) == R.L2_INF
        assert col.tie_group(z - 1) == (1, z) and col.tie_group(z) == (1, z) and col.tie_group(z + 1) == (z + 1, z + 20)
        assert col.tie_group(192)[1] > 192 and col.tie_group(257)[1] > 257              # ranks inside subnormal groups
        assert col.tie_group(ranks[3]) == (z + 121, z + 140) and col.tie_group(ranks[4])[0] == z + 141   # just past the subnormals
        if col.n == 1023:
            assert len(col.answer(col.n)[0]) == col.n - R.L2_INF
    for name in ("cosine-1023x64", "cosine-14003x64"):
        q, col, ranks = stores[name][2]["cosine"]
        n0, n1 = (4 * col.n) // 10, (3 * col.n) // 10
        assert np.sum(col.d == 0) == n0 and np.sum(col.d == 1) == n1 and np.sum(col.d == 2) == col.n - n0 - n1
        assert np.sum((col.d == 1) & (col.x != 0)) == n1 // 3                           # rows at or below the 1e-6 norm floor
        assert np.all(np.abs(np.log2(np.abs(col.x[col.x != 0]))) <= 60)
        assert ranks == (n0 - 1, n0, n0 + 1, n0 + n1 - 1, n0 + n1, n0 + n1 + 1) and ranks[-1] <= R.MAX_RESULTS
        assert col.tie_group(n0) == (1, n0) and col.tie_group(n0 + 1) == (n0 + 1, n0 + n1) and col.tie_group(n0 + n1 + 1)[0] == n0 + n1 + 1


# ---- one line of the kernels reverted: which GPU case notices -------------------------------------------------------------------

def wrong(col, k, rb, grid, defect):
    keys, _, _ = R.radix_select(col.d, rb, min(R.clamp_topk(k), col.n), grid, defect)
    return keys is None or not np.array_equal(keys, R.model_keys(col, k, rb))


REVERTS = {
    # defect -> GPU cases (store, column, k, row_base, select_grid) whose answer it changes. Routes (c) and (d) run every one of
    # them through the radix passes; route (b) those with k > 192 as well.
    "no_tail": [("dot-70001x64", "straddle-200", 200, 0, 0), ("dot-70001x64", "straddle-300", 1000, 0x00FFFF00, 4),
                ("dot-1023x64", "flat", 1023, 0, 0), ("dot-193x64", "wide", 194, 0xFFFE0000, 1)],
    "all_needed_zeros": [("dot-70001x64", "straddle-200", 200, 0, 0), ("dot-70001x64", "straddle-300", 300, 0xFFFE0000, 4),
                         ("dot-70001x64", "flat", 4096, 0, 0)],
    "no_prefix_match": [("dot-70001x64", "wide", 10, 0, 0), ("dot-70001x64", "around-zero", 1000, 0, 0),
                        ("dot-70001x64", "ladder-carry", 193, 0x00FFFF00, 4), ("l2-70001x64", "l2", 257, 0, 0)],
    "four_deep_i4": [("dot-70001x64", "flat", 10, 0, 4), ("dot-70001x64", "flat", 10000, 0x00FFFF00, 1),
                     ("dot-70001x64", "straddle-66000", 193, 0, 4), ("dot-70001x5-a", "flat", 1000, 0xFFFE0000, 4)],
}


@pytest.mark.parametrize("defect", list(REVERTS))
def test_a_reverted_line_changes_a_gpu_case(stores, defect):
    for name, cname, k, rb, grid in REVERTS[defect]:
        col = stores[name][2][cname][1]
        assert k in R.ks_of(cname, col, stores[name][2][cname][2]) and rb in R.row_bases_for(col.n)
        assert not wrong(col, k, rb, grid, None)
        assert wrong(col, k, rb, grid, defect), (defect, name, cname, k, rb, grid)


def test_four_deep_index_needs_the_small_grid_or_the_large_store(stores):
    """At the default grid 70 001 rows never enter the four-deep loop, so its row index shows only under select_grid 4 / 1 — and at
    the default grid on the one large case: there its first thread's rows 2 097 152.., 4 194 304.. and 6 291 456.. would be counted
    as rows 0..3, which the `flat` column of that store (the answer is rows 0 .. k - 1) turns into a wrong count."""
    col = stores["dot-70001x64"][2]["flat"][1]
    assert not wrong(col, 10, 0, 0, "four_deep_i4")
    d = np.full(R.BIG_N, 0.75, dtype=np.float32)
    assert R.radix_select(d, 0, 300, 0, "four_deep_i4")[0] is None
    keys, _, _ = R.radix_select(d, 0, 300, 0, None)
    assert np.array_equal(keys & np.uint64(0xffffffff), np.arange(300, dtype=np.uint64))


def test_dropping_the_early_exit_changes_no_answer(stores):
    """Removing the `all_needed` branch altogether (every query runs all eight passes and ends on the exact k-th key) is a cost, not
    an error: no answer can show it. What the answers pin is the branch's threshold (`all_needed_zeros` above: the ones below the
    decided digits) and its condition (`left == mine`)."""
    for name, cname, k, rb, grid in REVERTS["all_needed_zeros"]:
        col = stores[name][2][cname][1]
        assert not wrong(col, k, rb, grid, "no_all_needed")
        assert R.radix_select(col.d, rb, k, grid, "no_all_needed")[1] == 7
