"""The yardstick of the grouped search (tests/grouped_ref.py) proved before anything trusts it, and the boundary of the feature as
far as it can be seen without a GPU: the case tables hold the ties they claim, the crowded corpus defeats the over-fetch the
reference's callers use, the handle's merge is exact, and header, binding and library agree on the new entries."""
import ctypes

import numpy as np
import pytest

import grouped_ref as ref


def _groups_by_bits(case):
    """bits -> [(root, best row)] over the groups of a probe case."""
    keys = ref.make_keys(case.dist)
    full = ref.grouped_model(keys, case.parents, case.frame_ids, case.passing, 1 << 30, 1)
    out = {}
    for root, b, k in zip(full.roots.tolist(), full.bits.tolist(), full.member_keys[:, 0].tolist()):
        out.setdefault(b, []).append((root, int(k) & 0xffffffff))
    return out


# (the limit-1 case ranks one group, whose distance no other shares: it is there for the limit, not for a tie)
TIE_CASES = [c for c in ref.PROBE_CASES if c.name.startswith(("tied-blocks", "all-equal")) and c.limit > 1]


@pytest.mark.parametrize("case", TIE_CASES, ids=lambda c: c.name)
def test_tie_cases_hold_groups_whose_root_order_differs_from_their_rows(case):
    """Two groups with equal distance bits whose order by root id is the reverse of the order of their best rows, inside the part of
    the ranking the case asks for or at its edge: a selection that broke ties by row would answer differently."""
    exp = ref.probe_expected(case)
    asked = set(exp.bits.tolist())
    found = False
    for b, members in _groups_by_bits(case).items():
        if b not in asked or len(members) < 2:
            continue
        by_root = sorted(members)
        by_row = sorted(members, key=lambda m: m[1])
        found = found or by_root != by_row
    assert found


@pytest.mark.parametrize("case", [c for c in TIE_CASES if c.per_group > 1], ids=lambda c: c.name)
def test_within_group_tie_cases_have_equal_bits_at_two_rows(case):
    exp = ref.probe_expected(case)
    found = False
    for row in exp.member_keys:
        ks = row[row != ref.KEY_PAD]
        bits = ref.key_bits(ks)
        if len(ks) >= 2 and (bits[1:] == bits[:-1]).any():
            assert (np.diff(ref.key_rows(ks))[bits[1:] == bits[:-1]] > 0).all()   # equal bits: ascending rows
            found = True
    assert found


def test_root_ids_compare_unsigned():
    case = next(c for c in ref.PROBE_CASES if c.name.startswith("all-equal"))
    exp = ref.probe_expected(case)
    assert (exp.roots >= np.uint64(1 << 63)).all() and (np.diff(exp.roots.astype(object)) > 0).all()
    assert len(set(exp.bits.tolist())) == 1


def test_nonfinite_rows_take_no_part():
    case = next(c for c in ref.PROBE_CASES if c.name.startswith("signs"))
    keys = ref.make_keys(case.dist)
    assert (keys[~np.isfinite(case.dist)] == ref.KEY_PAD).all() and (~np.isfinite(case.dist)).sum() >= 20
    exp = ref.probe_expected(case)
    rows = ref.key_rows(exp.member_keys[exp.member_keys != ref.KEY_PAD])
    assert np.isfinite(case.dist[rows]).all()
    assert (np.diff(exp.bits.astype(np.int64)) >= 0).all() and exp.bits[0] < 0     # negative distances rank first; -0 below +0
    assert ref.order_bits(np.float32(-0.0)) < ref.order_bits(np.float32(0.0))


def crowded_corpus(limit, per_group, seed=3):
    """One root owns more than 8 * limit * per_group of the best rows: the reference's over-fetch sees nothing else."""
    rng = np.random.default_rng(seed)
    top_k = max(400, 8 * limit * per_group)
    n_crowd = top_k + 50
    n = n_crowd + 2000
    dist = np.empty(n, dtype=np.float32)
    dist[:n_crowd] = np.float32(0.01) + rng.random(n_crowd, dtype=np.float32) * np.float32(0.01)   # the long video: every segment close
    dist[n_crowd:] = np.float32(0.2) + rng.random(n - n_crowd, dtype=np.float32) * np.float32(0.5)
    parents = np.empty(n, dtype=np.uint64)
    parents[:n_crowd] = np.uint64(900_000)
    parents[n_crowd:] = np.uint64(1_000_000) + (np.arange(n - n_crowd, dtype=np.uint64) // np.uint64(10))
    perm = rng.permutation(n)
    return dist[perm], parents[perm], np.arange(n, dtype=np.uint64), top_k


@pytest.mark.parametrize("limit,per_group", [(12, 3), (12, 1), (30, 2)])
def test_crowded_corpus_defeats_the_over_fetch(limit, per_group):
    """Why the feature exists: collapsing the top max(400, 8 * limit * per_group) rows returns fewer than `limit` roots while the
    exact answer has `limit`."""
    dist, parents, fids, top_k = crowded_corpus(limit, per_group)
    keys = ref.make_keys(dist)
    exact = ref.grouped_model(keys, parents, fids, None, limit, per_group)
    today = ref.collapse_prefix(keys, parents, fids, None, top_k, limit)
    assert len(exact.roots) == limit
    assert len(today) < limit
    assert exact.roots[0] == np.uint64(900_000) and (exact.counts == per_group).all()


@pytest.mark.parametrize("seed", range(6))
def test_handle_merge_is_exact_on_random_splits(seed):
    """Every shard answers `limit` groups, the host keeps the smaller distance per root and sorts by (distance, root id): the global
    answer, whatever the split — a root among the global first `limit` is, on the shard that holds its best row, beaten only by
    roots that beat it globally."""
    rng = np.random.default_rng(50 + seed)
    n, limit = 3000, (1, 12, 200)[seed % 3]
    dist = (rng.integers(0, 64, size=n) / 64.0).astype(np.float32)            # few distinct values: ties across shards and roots
    fids = rng.permutation(n).astype(np.uint64)
    parents = rng.integers(0, 400, size=n).astype(np.uint64) + np.uint64(10_000)   # groups straddle the shards
    parents[rng.random(n) < 0.2] = ref.NO_PARENT
    keys = ref.make_keys(dist)
    glob = ref.grouped_model(keys, parents, fids, None, limit, 1)
    cuts = np.sort(rng.integers(0, n + 1, size=2))
    bounds = [0, int(cuts[0]), int(cuts[1]), n]
    answers, member_ids = [], {}
    for s in range(3):
        lo, hi = bounds[s], bounds[s + 1]
        a = ref.grouped_model(ref.make_keys(dist[lo:hi]), parents[lo:hi], fids[lo:hi], None, limit, 1)
        answers.append(a)
        for root, b, k in zip(a.roots.tolist(), a.bits.tolist(), a.member_keys[:, 0].tolist()):
            if root not in member_ids or b < member_ids[root][0]:
                member_ids[root] = (b, int(fids[lo + (int(k) & 0xffffffff)]))
    roots, bits = ref.merge_shards(answers, limit)
    assert np.array_equal(roots, glob.roots) and np.array_equal(bits, glob.bits)
    exp_members = fids[ref.key_rows(glob.member_keys[:, 0])]
    assert [member_ids[r][1] for r in roots.tolist()] == exp_members.tolist()   # contiguous shards: the lower shard is the lower row


def test_cut_drops_groups_and_members():
    dist = np.array([0.1, 0.2, 0.3, 0.6, 0.7, 0.15], dtype=np.float32)
    parents = np.array([1, 1, 1, 2, 2, 3], dtype=np.uint64)
    ans = ref.grouped_model(ref.make_keys(dist), parents, np.arange(6, dtype=np.uint64), None, 10, 3)
    assert ans.roots.tolist() == [1, 3, 2] and ans.counts.tolist() == [3, 1, 2]
    cut = ref.apply_cut(ans, np.float32(0.75))                                  # scores 0.9 0.8 0.7 | 0.85 | 0.4 0.3
    assert cut.roots.tolist() == [1, 3] and cut.counts.tolist() == [2, 1]
    assert ref.key_rows(cut.member_keys[0, :2]).tolist() == [0, 1] and cut.member_keys[0, 2] == ref.KEY_PAD


def test_slots_number_roots_densely():
    parents, fids = ref.partition("scattered", 500)
    slots, slot_root = ref.slots_of(parents, fids)
    roots = ref.roots_of(parents, fids)
    assert np.array_equal(slot_root[slots], roots) and len(set(slot_root.tolist())) == len(slot_root) == int(slots.max()) + 1


# ---- the boundary, without a GPU ----------------------------------------------------------------------------------------------

NEW = ("wax_hip_set_parents", "wax_hip_get_parents", "wax_hip_search_grouped", "wax_hip_group_stats", "wax_hip_group_probe")


def test_entries_are_declared_bound_and_exported(hip_lib):
    from wax_amd import _abi
    text = " ".join(open(_abi.HEADER_PATH).read().split())
    for name in NEW:
        assert name in _abi.declared_symbols() and name in _abi.SIGNATURES and hasattr(hip_lib, name)
    assert ("int wax_hip_search_grouped(wax_hip_engine* e, const float* query, uint32_t dims, int32_t limit, int32_t per_group, "
            "int has_min_score, float min_score, const wax_hip_row_predicate* pred, uint64_t* out_root_ids, float* out_root_scores, "
            "uint64_t* out_member_ids, float* out_member_scores, uint32_t* out_member_counts, uint32_t* out_count);") in text
    assert len(_abi.SIGNATURES["wax_hip_search_grouped"][1]) == 14 and len(_abi.SIGNATURES["wax_hip_group_probe"][1]) == 13
    assert "#define WAX_HIP_NO_PARENT UINT64_MAX" in text and "#define WAX_HIP_GROUP_MAX_LIMIT 1024" in text
    assert "#define WAX_HIP_GROUP_MAX_MEMBERS 8" in text
    assert _abi.NO_PARENT == int(ref.NO_PARENT) and _abi.GROUP_MAX_LIMIT == ref.MAX_LIMIT and _abi.GROUP_MAX_MEMBERS == ref.MAX_MEMBERS
    assert ctypes.sizeof(_abi.GroupStats) == 48
    assert hip_lib.wax_hip_abi_version() == 2


def test_null_arguments_are_refused_before_any_device(hip_lib):
    from wax_amd import _abi
    n = ctypes.c_uint32(77)
    roots = (ctypes.c_uint64 * 2)(5, 5)
    scores = (ctypes.c_float * 2)(5.0, 5.0)
    q = (ctypes.c_float * 4)()
    rc = hip_lib.wax_hip_search_grouped(None, q, 4, 2, 1, 0, 0.0, None, roots, scores, None, None, None, ctypes.byref(n))
    assert rc == _abi.ERR_INVALID_ARGUMENT and "null" in _abi.last_error() and n.value == 77 and list(roots) == [5, 5]
    applied = ctypes.c_uint64(9)
    assert hip_lib.wax_hip_set_parents(None, roots, roots, 2, ctypes.byref(applied)) == _abi.ERR_INVALID_ARGUMENT
    assert hip_lib.wax_hip_get_parents(None, roots, 2, roots, None) == _abi.ERR_INVALID_ARGUMENT and list(roots) == [5, 5]
    assert hip_lib.wax_hip_group_stats(None, None) == _abi.ERR_INVALID_ARGUMENT
    keys = (ctypes.c_int64 * 2)(3, 3)
    d = (ctypes.c_float * 4)()
    # the probe's refusals come before its first device call
    for limit, per in ((2000, 1), (2, 9), (2, 0)):
        rc = hip_lib.wax_hip_group_probe(d, None, None, None, 4, 4, limit, per, 0, roots, keys, None, ctypes.byref(n))
        assert rc == _abi.ERR_INVALID_ARGUMENT and n.value == 77 and list(keys) == [3, 3]
    assert hip_lib.wax_hip_group_probe(d, None, None, None, 4, 3, 2, 1, 0, roots, keys, None, ctypes.byref(n)) == _abi.ERR_INVALID_ARGUMENT
    assert hip_lib.wax_hip_group_probe(d, None, None, None, 4, 4, 0, 1, 0, roots, keys, None, ctypes.byref(n)) == _abi.OK and n.value == 0
