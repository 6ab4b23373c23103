"""The batched required-term search without a device: the bit-sliced model of term_mask_multi_kernel (tests/batch_terms_ref.py) held to
set containment — exhaustively on small universes, and at sets of 15 and 16 terms and rows of 64; the new symbols in the header and in
_abi.py; the refusals that come before any device call; how searchBatchTerms reads requiredTerms, NO_MATCH included."""
import ctypes
import itertools

import numpy as np
import pytest

import batch_terms_ref as bref
import terms_ref as ref


def csr(rows):
    return ref.csr_of(rows)


def test_bit_sliced_model_is_containment_on_every_row_of_a_small_universe():
    """Universe 0 .. 6: every one of the 128 rows against groups of sets that cover every non-empty subset of the universe once."""
    universe = range(7)
    rows = [tuple(t for t in universe if (m >> t) & 1) for m in range(128)]
    off, val = csr(rows)
    subsets = [s for m in range(1, 128) for s in [tuple(t for t in universe if (m >> t) & 1)]]
    for g0 in range(0, len(subsets), 32):
        sets = subsets[g0:g0 + 32]
        got, exp = bref.multi_model(off, val, sets), bref.containment(off, val, sets)
        assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]), g0
        for s, req in enumerate(sets):                               # and containment is what it says: a plain subset test per row
            assert ref.bits_of(exp[0][s], 128).tolist() == [set(req) <= set(r) for r in rows]


def test_bit_sliced_model_on_every_pair_and_triple_of_sets_of_a_tiny_universe():
    """Universe 0 .. 3, 16 rows: every ordered pair and triple of non-empty sets — subsets of one another, equal sets, disjoint ones."""
    rows = [tuple(t for t in range(4) if (m >> t) & 1) for m in range(16)]
    off, val = csr(rows)
    subsets = [tuple(t for t in range(4) if (m >> t) & 1) for m in range(1, 16)]
    for r in (2, 3):
        for sets in itertools.product(subsets, repeat=r):
            got, exp = bref.multi_model(off, val, sets), bref.containment(off, val, sets)
            assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]), sets


@pytest.mark.parametrize("family", ("disjoint16", "shared"))
@pytest.mark.parametrize("n_sets", (1, 2, 31, 32))
def test_bit_sliced_model_at_fifteen_and_sixteen_terms_and_rows_of_64(family, n_sets):
    rng = np.random.default_rng(n_sets * 7 + len(family))
    sets = bref.make_sets(family, n_sets, rng)
    sizes = {len(s) for s in sets}
    assert 16 in sizes and (family == "disjoint16" or n_sets < 4 or {1, 2, 15, 16} <= sizes)
    rows, kinds = bref.make_rows(sets, 1200, rng)
    assert max(len(r) for r in rows) == 64 and min(len(r) for r in rows) == 0 and set(kinds) == set(bref.KINDS)
    assert all(list(r) == sorted(set(r)) for r in rows)
    off, val = csr(rows)
    got, exp = bref.multi_model(off, val, sets), bref.containment(off, val, sets)
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])
    assert exp[1].all()                                                # every set has rows that pass it
    # a row one term short of a set does not pass it; a row that spreads |set s| union terms over two sets passes neither of them
    w = bref.pass_words(off, val, sets)
    for r, kind in enumerate(kinds):
        held = [s for s in range(n_sets) if set(sets[s]) <= set(rows[r])]
        assert [s for s in range(n_sets) if (int(w[r]) >> s) & 1] == held
    if family == "disjoint16":
        u, memb, nbits, live = bref.plan(sets)
        assert len(u) == 16 * n_sets and (n_sets < 32 or len(u) == bref.MAX_UNION)
        assert int(live) == (1 << n_sets) - 1 and int(nbits[4]) == int(live) and not nbits[:4].any()
        spread = [r for r, kind in enumerate(kinds) if kind == "spread" and len(rows[r]) == 16]
        assert n_sets == 1 or (spread and all(int(w[r]) == 0 for r in spread))
    else:
        common = set.intersection(*[set(s) for s in sets])
        assert len(common) >= 1 and (n_sets < 2 or set(sets[1]) < set(sets[0]))


def test_plan_words():
    u, memb, nbits, live = bref.plan([[5, 9], [9], [9, 5, 7, 7]])
    assert u.tolist() == [5, 7, 9] and memb.tolist() == [0b101, 0b100, 0b111] and int(live) == 0b111
    assert nbits.tolist() == [0b110, 0b101, 0, 0, 0]                # sizes 2, 1, 3


def test_header_and_abi_carry_the_new_symbols(hip_lib):
    from wax_amd import _abi
    text = " ".join(open(_abi.HEADER_PATH).read().split())
    for name in ("wax_hip_search_batch_terms", "wax_hip_term_batch_stats", "wax_hip_term_mask_multi_probe"):
        assert name in _abi.declared_symbols() and name in _abi.SIGNATURES and hasattr(hip_lib, name)
    assert "#define WAX_HIP_ABI_VERSION 2" in text and hip_lib.wax_hip_abi_version() == 2
    assert len(_abi.SIGNATURES["wax_hip_search_batch_terms"][1]) == len(_abi.SIGNATURES["wax_hip_search_batch_predicate"][1]) + 4 == 19
    assert len(_abi.SIGNATURES["wax_hip_term_mask_multi_probe"][1]) == 10
    assert ctypes.sizeof(_abi.TermBatchStats) == 48 and ctypes.sizeof(_abi.TermStats) == 48      # wax_hip_term_stats_t did not grow
    assert [n for n, _ in _abi.TermBatchStats._fields_] == ["calls", "queries", "sets", "mask_launches", "looped", "host_decided"]
    hpp = open(_abi.HEADER_PATH.replace("wax_hip.h", "wax_hip.hpp")).read()
    for name in ("wax_hip_set_terms", "wax_hip_get_terms", "wax_hip_search_terms", "wax_hip_search_batch_terms", "wax_hip_term_stats",
                 "wax_hip_term_batch_stats"):
        assert name in hpp, name


def test_refusals_that_need_no_device(hip_lib):
    from wax_amd import _abi
    u32, u64, f32 = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_float
    q = (f32 * 8)(*([1.0] * 8))
    ids, scores, counts = (u64 * 4)(5, 5, 5, 5), (f32 * 4)(2, 2, 2, 2), (u32 * 2)(77, 77)
    terms, begin, length = (u32 * 2)(3, 4), (u64 * 2)(0, 1), (u32 * 2)(1, 1)
    # a null engine is refused first, with or without term arrays, and the outputs stay
    for tb, tl in ((begin, length), (None, None), (begin, None)):
        rc = hip_lib.wax_hip_search_batch_terms(None, q, 2, 4, 2, None, 0, None, None, None, None, terms, 2, tb, tl, ids, scores, 2, counts)
        assert rc == _abi.ERR_INVALID_ARGUMENT and "engine is null" in _abi.last_error()
        assert list(counts) == [77, 77] and list(ids) == [5, 5, 5, 5] and list(scores) == [2, 2, 2, 2]
    assert hip_lib.wax_hip_term_batch_stats(None, None) == _abi.ERR_INVALID_ARGUMENT
    # the probe's refusals come before its first device call
    off, val = (u32 * 3)(0, 1, 2), (u32 * 2)(4, 4)
    out, cnt = (u32 * 2)(123, 123), (u32 * 2)(9, 9)
    req17, b0 = (u32 * 17)(*range(17)), (u64 * 1)(0)

    def probe(off_=off, req=req17, beg=b0, ln=1, n_sets=1, grid=1, rows=2):
        return hip_lib.wax_hip_term_mask_multi_probe(off_, val, rows, req, beg, (u32 * 1)(ln) if ln is not None else None, n_sets, grid, out, cnt)
    assert probe(ln=17) == _abi.ERR_INVALID_ARGUMENT and "more than 16" in _abi.last_error()
    assert probe(ln=0) == _abi.ERR_INVALID_ARGUMENT and "empty" in _abi.last_error()
    assert probe(n_sets=0) == _abi.ERR_INVALID_ARGUMENT and probe(n_sets=33) == _abi.ERR_INVALID_ARGUMENT
    assert "1 to 32 term sets" in _abi.last_error()
    assert probe(grid=0) == _abi.ERR_INVALID_ARGUMENT and probe(grid=1025) == _abi.ERR_INVALID_ARGUMENT
    assert probe(rows=0) == _abi.ERR_INVALID_ARGUMENT
    assert probe(off_=(u32 * 3)(0, 2, 1)) == _abi.ERR_INVALID_ARGUMENT and "must not decrease" in _abi.last_error()
    assert probe(off_=None) == _abi.ERR_INVALID_ARGUMENT and probe(ln=None) == _abi.ERR_INVALID_ARGUMENT
    assert list(out) == [123, 123] and list(cnt) == [9, 9]


def _recorder():
    """Stands in for an engine: records what searchBatchTerms sends to wax_hip_search_batch_terms and answers query i of the call
    with one hit, id 100 + i."""
    from wax_amd import HIPVectorEngine

    class Lib:
        def __init__(self):
            self.calls = []

        def wax_hip_search_batch_terms(self, *args):
            self.calls.append(args)
            n, kcap = args[2], args[17]
            u64 = ctypes.cast(args[15], ctypes.POINTER(ctypes.c_uint64))
            cnt = ctypes.cast(args[18], ctypes.POINTER(ctypes.c_uint32))
            for i in range(n):
                u64[i * kcap] = 100 + i
                cnt[i] = 1
            return 0

        def __getattr__(self, name):
            raise AssertionError(f"unexpected call of {name}")

    class Recorder(HIPVectorEngine):
        count = 1000

        def __init__(self):
            self._lib = Lib()
            self._h = None

        @property
        def calls(self):
            return self._lib.calls
    return Recorder()


def _u32s(ptr, n):
    return [ctypes.cast(ptr, ctypes.POINTER(ctypes.c_uint32))[i] for i in range(n)]


def _u64s(ptr, n):
    return [ctypes.cast(ptr, ctypes.POINTER(ctypes.c_uint64))[i] for i in range(n)]


def test_python_layer_packs_term_filters_and_never_sends_a_no_match_query():
    from wax_amd import TermDictionary
    from wax_amd.errors import EncodingError
    nm = TermDictionary.NO_MATCH
    qs = np.arange(5 * 4, dtype=np.float32).reshape(5, 4)
    call = lambda eng, requiredTerms, **kw: eng.searchBatchTerms(qs, 3, requiredTerms, **kw)   # noqa: E731,N803
    # per query: ids, NO_MATCH, None, an empty filter, ids as an array
    eng = _recorder()
    ids, scores, counts = call(eng, requiredTerms=[[7, 8], nm, None, [], np.array([9], dtype=np.uint32)],
                               frameIds=[None, [1], [2, 3], None, None], minScore=[0.5, None, 0.25, None, None])
    (args,) = eng.calls
    assert args[2] == 4 and args[3] == 4                                                # four queries sent: query 1 is not among them
    sent = np.ctypeslib.as_array(ctypes.cast(args[1], ctypes.POINTER(ctypes.c_float)), shape=(4, 4))
    assert np.array_equal(sent, qs[[0, 2, 3, 4]])
    assert args[12] == 3 and _u32s(args[11], 3) == [7, 8, 9]
    assert _u64s(args[13], 4) == [0, 2, 2, 2] and _u32s(args[14], 4) == [2, 0, 0, 1]
    assert args[6] == 2 and _u64s(args[5], 2) == [2, 3]                                 # the dropped query's list is not packed either
    cuts = np.ctypeslib.as_array(ctypes.cast(args[9], ctypes.POINTER(ctypes.c_float)), shape=(4,))
    assert cuts[0] == 0.5 and cuts[1] == 0.25 and np.isnan(cuts[2:]).all()
    assert counts.tolist() == [1, 0, 1, 1, 1] and ids[:, 0].tolist() == [100, 0, 101, 102, 103]
    # one filter for all queries; NO_MATCH for all: no call at all
    eng = _recorder()
    call(eng, requiredTerms=[4, 5])
    (args,) = eng.calls
    assert args[2] == 5 and _u32s(args[14], 5) == [2] * 5 and _u32s(args[11], 10) == [4, 5] * 5
    eng = _recorder()
    ids, scores, counts = call(eng, requiredTerms=nm)
    assert eng.calls == [] and counts.tolist() == [0] * 5 and ids.shape == (5, 3)
    eng = _recorder()
    assert call(eng, requiredTerms=[nm] * 5)[2].tolist() == [0] * 5 and eng.calls == []
    # a per-query timeRange / denyFlags follows its query past the dropped one
    eng = _recorder()
    call(eng, requiredTerms=[nm, [1], [1], [1], [1]], denyFlags=[1, 2, 0, 0, 4], timeRange=[None, (1, 2), None, None, None])
    (args,) = eng.calls
    preds = args[10]
    assert [preds[i].deny_flags for i in range(4)] == [2, 0, 0, 4] and (preds[0].has_after, preds[0].after, preds[0].before) == (1, 1, 2)
    # wrong lengths raise before any call
    eng = _recorder()
    for bad in ([[1], [2]], [None] * 6):
        with pytest.raises(EncodingError, match="requiredTerms"):
            call(eng, requiredTerms=bad)
    with pytest.raises(EncodingError, match="frameIds"):
        call(eng, requiredTerms=[1], frameIds=[None])
    assert eng.calls == []
