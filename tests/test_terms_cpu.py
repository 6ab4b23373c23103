"""The required-term search without a device: the numpy model of its contract (tests/terms_ref.py) against
matches(metadataFilter:meta:) restated from UnifiedSearch.swift:1215-1239 on a hand-written fixture; the corpus on which the
reference's post-filter of an over-fetched prefix returns too few hits while the pre-filter returns k; the new symbols in the header
and in _abi.py; the refusals that come before any device call; TermDictionary."""
import ctypes

import numpy as np
import pytest

import terms_ref as ref

# entries (None: the frame has no metadata), tags, labels
FRAMES = [
    ({"session_id": "a", "lang": "en"}, [("topic", "gpu")], ["pinned"]),
    ({"session_id": "b", "lang": "en"}, [("topic", "gpu"), ("topic", "hip")], []),
    ({"session_id": "a"}, [], ["pinned", "draft"]),
    (None, [("topic", "gpu")], ["pinned"]),
    ({}, [], []),
    ({"session_id": "a", "lang": "de"}, [("topic", "hip")], ["draft"]),
    ({"lang": "a", "session_id": "en"}, [("gpu", "topic")], ["session_id"]),       # the same strings in other places
]
FILTERS = [
    ({}, [], []),
    ({"session_id": "a"}, [], []),
    ({"session_id": "a", "lang": "en"}, [], []),
    ({}, [("topic", "gpu")], []),
    ({}, [("topic", "gpu"), ("topic", "hip")], []),
    ({}, [], ["pinned"]),
    ({"session_id": "a"}, [("topic", "gpu")], ["pinned"]),
    ({"session_id": "a"}, [], ["draft", "pinned"]),
    ({"session_id": "zzz"}, [], []),                                               # never interned
    ({}, [("topic", "nobody")], []),
    ({}, [], ["nobody"]),
    ({"lang": "a"}, [], ["session_id"]),
]


def test_term_model_agrees_with_the_restated_metadata_filter():
    from wax_amd import TermDictionary
    d = TermDictionary()
    sets = [d.forFrame(e, t, l) for e, t, l in FRAMES]
    assert all(len(s) == len(set(s)) and list(s) == sorted(s) for s in sets)
    seen_true = seen_false = 0
    for re_, rt, rl in FILTERS:
        want = np.array([ref.matches_metadata_filter(re_, rt, rl, e, t, l) for e, t, l in FRAMES])
        req = d.forFilter(requiredEntries=re_, requiredTags=rt, requiredLabels=rl)
        if req is TermDictionary.NO_MATCH:
            assert not want.any(), (re_, rt, rl)
            continue
        got = ref.pass_set(sets, req)
        assert np.array_equal(got, want), (re_, rt, rl)
        seen_true += int(want.sum())
        seen_false += int((~want).sum())
    assert seen_true > 5 and seen_false > 5
    n = len(d)
    assert d.forFilter(requiredEntries={"session_id": "zzz"}) is TermDictionary.NO_MATCH and len(d) == n   # a filter interns nothing


def test_term_dictionary_round_trips():
    from wax_amd import TermDictionary
    d = TermDictionary()
    a, b, c = d.entry("k", "v"), d.tag("k", "v"), d.label("k")
    assert len({a, b, c}) == 3 and d.entry("k", "v") == a and d.tag("k", "v") == b and d.label("k") == c and len(d) == 3
    assert d.lookup(a) == ("entry", "k", "v") and d.lookup(b) == ("tag", "k", "v") and d.lookup(c) == ("label", "k")
    assert d.forFilter() == [] and d.forFilter(requiredEntries={"k": "v"}, requiredTags=[("k", "v")], requiredLabels=["k"]) == sorted([a, b, c])
    assert d.forFilter(requiredEntries={"k": "w"}) is TermDictionary.NO_MATCH
    assert d.forFilter(requiredLabels=["k", "k"]) == [c]
    assert d.forFrame({"k": "v"}, [("k", "v"), ("k", "v")], ["k", "new"]) == sorted([a, b, c, 3]) and len(d) == 4
    assert all(0 <= t < 2**32 for t in (a, b, c))


def test_bitmap_model_helpers_round_trip():
    rng = np.random.default_rng(3)
    for n in (1, 31, 32, 33, 64, 65, 257):
        p = rng.random(n) < 0.4
        bm = ref.bitmap_of(p)
        assert bm.dtype == np.uint32 and len(bm) == (n + 31) // 32 and np.array_equal(ref.bits_of(bm, n), p)
    off, val = ref.csr_of([(5, 3, 5), (), (9,)])
    assert off.tolist() == [0, 2, 2, 3] and val.tolist() == [3, 5, 9]
    assert ref.mask_model([(1, 2), (2,), (1, 2, 3)], [1, 2]).tolist() == [0b101]
    assert ref.mask_model([(1, 2), (2,), (1, 2, 3)], [2], bitmap_in=np.array([0b110], dtype=np.uint32)).tolist() == [0b110]


def test_post_filter_of_the_prefix_starves_a_small_session_and_the_pre_filter_does_not():
    """1 000 rows, the session owns every 50th; the 30 best rows overall are other sessions' except one."""
    n, k = 1000, 10
    rng = np.random.default_rng(7)
    scores = rng.random(n).astype(np.float32) * 0.5
    session = 7
    sets = [(100 + int(i % 50), 3) for i in range(n)]                       # term 100 + s: the session; 3: everybody
    mine = np.nonzero(ref.pass_set(sets, [100 + session]))[0]
    assert len(mine) == 20
    others = np.setdiff1d(np.arange(n), mine)
    scores[others[:40]] = 0.9 + rng.random(40).astype(np.float32) * 0.05    # they crowd the prefix
    scores[mine[0]] = 0.99
    passing = ref.pass_set(sets, [100 + session, 3])
    post = ref.post_filter_rows(scores, passing, k)
    pre = ref.topk_rows(scores, passing, k)
    assert len(post) == 1 and post[0] == mine[0]                            # the reference: fewer than k
    assert len(pre) == k and pre[0] == mine[0] and passing[pre].all()       # the pre-filter: k
    assert np.all(np.diff(scores[pre]) <= 0)
    best_of_mine = np.sort(scores[mine])[::-1][:k]
    assert np.array_equal(scores[pre], best_of_mine)


def test_header_and_abi_carry_the_new_symbols(hip_lib):
    from wax_amd import _abi
    text = " ".join(open(_abi.HEADER_PATH).read().split())
    for name in ("wax_hip_set_terms", "wax_hip_get_terms", "wax_hip_search_terms", "wax_hip_term_stats", "wax_hip_term_mask_probe"):
        assert name in _abi.declared_symbols() and name in _abi.SIGNATURES and hasattr(hip_lib, name)
    assert "#define WAX_HIP_TERMS_MAX_PER_ROW 64" in text and "#define WAX_HIP_TERMS_MAX_REQUIRED 16" in text
    assert "#define WAX_HIP_ABI_VERSION 2" in text and hip_lib.wax_hip_abi_version() == 2
    assert _abi.TERMS_MAX_PER_ROW == ref.MAX_PER_ROW and _abi.TERMS_MAX_REQUIRED == ref.MAX_REQUIRED
    assert len(_abi.SIGNATURES["wax_hip_search_terms"][1]) == 16 and len(_abi.SIGNATURES["wax_hip_set_terms"][1]) == 8
    assert len(_abi.SIGNATURES["wax_hip_term_mask_probe"][1]) == 8 and ctypes.sizeof(_abi.TermStats) == 48
    assert "UnifiedSearch.swift:1215-1239" in text and "SearchRequest.swift:130-145" in text


def test_refusals_that_need_no_device(hip_lib):
    from wax_amd import _abi
    u32, u64 = ctypes.c_uint32, ctypes.c_uint64
    q = (ctypes.c_float * 4)(1, 0, 0, 0)
    ids = (u64 * 2)(5, 5)
    scores = (ctypes.c_float * 2)(0, 0)
    n = u32(77)
    one = (u32 * 1)(9)
    # null engine: the predicate search's refusal and message, the outputs untouched
    rc = hip_lib.wax_hip_search_terms(None, q, 4, 2, 0, None, 0, 0, 0.0, None, one, 1, ids, scores, 2, ctypes.byref(n))
    assert rc == _abi.ERR_INVALID_ARGUMENT and "engine is null" in _abi.last_error() and n.value == 0 and list(ids) == [5, 5]
    n = u32(77)
    rc = hip_lib.wax_hip_search_terms(None, q, 4, 2, 0, None, 0, 0, 0.0, None, None, 0, ids, scores, 2, ctypes.byref(n))   # no terms: search_predicate's
    assert rc == _abi.ERR_INVALID_ARGUMENT and "engine is null" in _abi.last_error()
    got, found, applied = u32(3), ctypes.c_uint8(3), u64(3)
    assert hip_lib.wax_hip_get_terms(None, 1, one, 1, ctypes.byref(got), ctypes.byref(found)) == _abi.ERR_INVALID_ARGUMENT
    assert got.value == 0 and found.value == 0
    assert hip_lib.wax_hip_term_stats(None, None) == _abi.ERR_INVALID_ARGUMENT
    # set_terms checks its arguments against themselves before it looks at the engine
    fid, beg = (u64 * 1)(1), (u64 * 1)(0)
    many = (u32 * 70)(*range(70))
    assert hip_lib.wax_hip_set_terms(None, fid, beg, (u32 * 1)(64), many, 70, 1, ctypes.byref(applied)) == _abi.ERR_INVALID_ARGUMENT
    assert "engine is null" in _abi.last_error() and applied.value == 0
    assert hip_lib.wax_hip_set_terms(None, fid, beg, (u32 * 1)(65), many, 70, 1, ctypes.byref(applied)) == _abi.ERR_INVALID_ARGUMENT
    assert "more than 64" in _abi.last_error()
    dup = (u32 * 70)(*([1] * 10 + list(range(60))))                          # 70 entries, 60 distinct: fine after de-duplication
    assert hip_lib.wax_hip_set_terms(None, fid, beg, (u32 * 1)(70), dup, 70, 1, ctypes.byref(applied)) == _abi.ERR_INVALID_ARGUMENT
    assert "engine is null" in _abi.last_error()
    for b, ln in ((0, 71), (70, 1), (71, 0), (2**63, 2)):
        rc = hip_lib.wax_hip_set_terms(None, fid, (u64 * 1)(b), (u32 * 1)(ln), many, 70, 1, ctypes.byref(applied))
        assert rc == _abi.ERR_INVALID_ARGUMENT and "leaves the term array" in _abi.last_error(), (b, ln)
    # the probe's refusals come before its first device call
    off, val, out = (u32 * 3)(0, 1, 2), (u32 * 2)(4, 4), (u32 * 1)(123)
    req17 = (u32 * 17)(*range(17))
    assert hip_lib.wax_hip_term_mask_probe(off, val, 2, req17, 17, None, 1, out) == _abi.ERR_INVALID_ARGUMENT
    assert "more than 16" in _abi.last_error() and out[0] == 123
    assert hip_lib.wax_hip_term_mask_probe(off, val, 2, req17, 0, None, 1, out) == _abi.ERR_INVALID_ARGUMENT
    assert hip_lib.wax_hip_term_mask_probe(off, val, 2, one, 1, None, 0, out) == _abi.ERR_INVALID_ARGUMENT
    assert hip_lib.wax_hip_term_mask_probe(off, val, 2, one, 1, None, 1025, out) == _abi.ERR_INVALID_ARGUMENT
    assert hip_lib.wax_hip_term_mask_probe((u32 * 3)(0, 2, 1), val, 2, one, 1, None, 1, out) == _abi.ERR_INVALID_ARGUMENT
    assert hip_lib.wax_hip_term_mask_probe(None, val, 2, one, 1, None, 1, out) == _abi.ERR_INVALID_ARGUMENT and out[0] == 123


def test_python_layer_answers_no_match_without_a_call():
    from wax_amd import HIPVectorEngine, TermDictionary
    ids, scores = HIPVectorEngine.searchFiltered(None, np.zeros(4, dtype=np.float32), 10, requiredTerms=TermDictionary.NO_MATCH)
    assert ids.dtype == np.uint64 and scores.dtype == np.float32 and len(ids) == 0 and len(scores) == 0


def test_made_up_columns_are_sorted_distinct_and_both_models_agree():
    rng = np.random.default_rng(11)
    n = 300
    lens = rng.integers(0, 65, size=n)
    c = np.where(rng.random(n) < 0.3, rng.integers(0, 17, size=n), 0)
    hc = (rng.random(n) < 0.5).astype(np.int64)
    lens = np.maximum(lens, 17)
    off, val = ref.build_column(lens, c, hc)
    sets = ref.sets_of(off, val)
    assert all(list(s) == sorted(set(s)) and len(s) <= ref.MAX_PER_ROW for s in sets)
    assert not any(ref.NOBODY in s for s in sets)
    for req in ([1], [1, 2], list(ref.SPECIALS), [ref.COMMON], [ref.NOBODY], [ref.COMMON, 16], [2, 2, 1]):
        assert np.array_equal(ref.pass_csr(off, val, req), ref.pass_set(sets, req)), req
    assert np.array_equal(ref.pass_csr(off, val, list(ref.SPECIALS)), c == 16) and np.array_equal(ref.pass_csr(off, val, [ref.COMMON]), hc == 1)
    off2, val2 = ref.csr_of(sets)
    assert np.array_equal(off2, off) and np.array_equal(val2, val)
