"""The batched required-term search on the device (wax_hip_search_batch_terms; term_mask_multi_kernel, wax_amd/csrc/terms.hip).

Probe: wax_hip_term_mask_multi_probe on made-up columns (tests/batch_terms_ref.py) against set containment — bitmaps and counts,
array_equal. Engine: searchBatchTerms(..., requiredTerms) against the loop of searchFiltered(requiredTerms=...) and against
searchBatchFiltered(frameIds = the ids the model passes), ids and score bits, array_equal."""
import ctypes

import numpy as np
import pytest

import batch_terms_ref as bref
import terms_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def wax():
    import wax_amd
    if not wax_amd.HIPVectorEngine.isAvailable():
        pytest.skip("no gfx950 device")
    return wax_amd


# ---- through the probe ------------------------------------------------------------------------------------------------------

ROWS = (1, 63, 64, 65, 257, 4097, 20_000)
GRIDS = (1, 2, 3)
BASE_ROWS = 1500        # distinct made-up rows per case; larger columns repeat them in random order


@pytest.fixture(scope="module")
def columns():
    """(family, n_sets) -> (sets, base rows, their kinds): made once, the cases of every row count draw from them."""
    made = {}

    def get(family, n_sets):
        key = (family, n_sets)
        if key not in made:
            rng = np.random.default_rng(1000 * n_sets + len(family))
            sets = bref.make_sets(family, n_sets, rng)
            rows, kinds = bref.make_rows(sets, BASE_ROWS, rng)
            made[key] = (sets, rows, kinds)
        return made[key]
    return get


@pytest.mark.parametrize("family", ("disjoint16", "shared"))
@pytest.mark.parametrize("n_sets", (1, 2, 31, 32))
@pytest.mark.parametrize("n", ROWS)
def test_probe_equals_set_containment(wax, columns, n, n_sets, family):
    sets, base, kinds = columns(family, n_sets)
    rng = np.random.default_rng(n * 31 + n_sets)
    pick = rng.permutation(len(base))[:n] if n <= len(base) else rng.integers(0, len(base), size=n)
    if n >= 257:                                                    # the row kinds the issue names are all there
        assert {kinds[i] for i in pick} == set(bref.KINDS)
    rows = [base[i] for i in pick]
    off, val = ref.csr_of(rows)
    assert n < 257 or int(np.diff(off.astype(np.int64)).max()) == 64
    exp_bm, exp_cnt = bref.containment(off, val, sets)
    if family == "disjoint16" and n_sets == 32:
        assert len({t for s in sets for t in s}) == bref.MAX_UNION  # a union of exactly 512 terms
    if n >= 257:
        assert exp_cnt.all() and (val < bref.LO).any() and (val >= bref.HI).any()   # values below U's first term and above its last
    for grid in GRIDS:
        bm, cnt = wax.termMaskMultiProbe(off, val, sets, grid=grid)
        assert np.array_equal(cnt, exp_cnt), (grid, cnt, exp_cnt)
        assert np.array_equal(bm, exp_bm), grid


def test_probe_named_rows(wax):
    """By hand: a term all 32 sets require; a set inside another; a row one term short; a row with |set s| union terms spread over two
    sets; rows of 0, 1 and 64 values; values below the union's first term and above its last."""
    common = 500
    sets = [[common] + [1000 + 20 * s + i for i in range(15)] for s in range(30)]          # 30 sets of 16
    sets.append(sets[0][:5])                                                              # set 30 inside set 0
    sets.append([common])                                                                 # set 31: the common term alone
    assert len(sets) == 32
    rows = [
        (),                                                                               # 0: no value
        (common,),                                                                        # 1: one value: set 31 only
        tuple(sets[0]),                                                                   # 2: set 0, hence 30 and 31
        tuple(sets[0][:-1]),                                                              # 3: set 0 less its last term: 30 and 31
        tuple(sets[3][1:]),                                                               # 4: set 3 without the common term: nothing
        tuple(sorted(sets[1][:8] + sets[2][8:])),                                         # 5: 16 union terms over sets 1 and 2: 31 alone
        tuple(sorted(sets[4] + list(range(1, 49)))),                                      # 6: 64 values, 48 of them below the union
        tuple(sorted(sets[5] + [2**32 - 1 - i for i in range(48)])),                      # 7: 64 values, 48 of them above it
        (1, 2, 3, 2**32 - 1),                                                             # 8: only values outside [first, last]
        tuple(sorted(set(sets[6]) | set(sets[7]) | set(sets[8]) | set(sets[9]))),         # 9: four whole sets (61 values)
        (1003,),                                                                          # 10: one value of the union that is no set
    ]
    want = {0: [], 1: [31], 2: [0, 30, 31], 3: [30, 31], 4: [], 5: [31], 6: [4, 31], 7: [5, 31], 8: [], 9: [6, 7, 8, 9, 31], 10: []}
    off, val = ref.csr_of(rows)
    assert [len(r) for r in rows][6:8] == [64, 64]
    for grid in GRIDS:
        bm, cnt = wax.termMaskMultiProbe(off, val, sets, grid=grid)
        got = {r: [s for s in range(32) if (int(bm[s][0]) >> r) & 1] for r in range(len(rows))}
        assert got == want
        assert cnt.tolist() == [sum(s in v for v in want.values()) for s in range(32)]
    mbm, mcnt = bref.multi_model(off, val, sets)
    assert np.array_equal(mbm, bm) and np.array_equal(mcnt, cnt)


# ---- through an engine ------------------------------------------------------------------------------------------------------

METRICS = ("cosine", "dot", "l2")
DIMS = 64
SESSION0, TAG0, EVERYBODY, NOBODY = 1000, 2000, 7, 8
SESSIONS = 40


def make_rows(n, seed):
    """Gaussian rows of which about a sixth repeat an earlier row bit for bit (equal scores, decided by row order), and 12 queries."""
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((n, DIMS)).astype(np.float32)
    dup = np.nonzero(rng.random(n) < 0.17)[0]
    dup = dup[dup > 0]
    rows[dup] = rows[rng.integers(0, dup)]
    return rows, rng.standard_normal((12, DIMS)).astype(np.float32)


def make_term_sets(n, seed):
    """Six terms per row: one of SESSIONS session ids, two tags of four, EVERYBODY, two private ones."""
    rng = np.random.default_rng(seed)
    ses, t1, t2 = rng.integers(0, SESSIONS, size=n), rng.integers(0, 4, size=n), rng.integers(0, 4, size=n)
    return [(SESSION0 + int(ses[r]), TAG0 + int(t1[r]), TAG0 + 10 + int(t2[r]), EVERYBODY, 100_000 + 2 * r, 100_001 + 2 * r) for r in range(n)]


class Store:
    def __init__(self, wax, metric, n, seed, devices=None, terms=True):
        self.wax, self.n = wax, n
        self.rows, self.queries = make_rows(n, seed)
        self.fids = np.random.default_rng(seed + 1).permutation(n).astype(np.uint64) * 3 + 5
        self.sets = make_term_sets(n, seed + 2) if terms else [()] * n
        self.ts = np.random.default_rng(seed + 3).integers(0, 100, size=n).astype(np.int64)
        self.fl = np.where(np.random.default_rng(seed + 4).random(n) < 0.2, 0x100, 0).astype(np.uint32)
        self.eng = wax.HIPVectorEngine(metric=getattr(wax.VectorMetric, metric), dimensions=DIMS, devices=devices)
        if devices:
            self.eng.setTuning("shard_min_mb", 0)
            self.eng.reserve(n)
        self.eng.addBatch(self.fids, self.rows)
        if terms:
            assert self.eng.setTerms(self.fids, self.sets) == n
        assert self.eng.setAttributes(self.fids, self.ts, self.fl) == n

    def model_ids(self, req, allow):
        """The frame ids the model passes for one query: the rows whose set holds `req`, among `allow` where that is a list."""
        ids = self.fids if req is None else self.fids[ref.pass_set(self.sets, req)]
        return ids if allow is None else ids[np.isin(ids, allow)]

    def check(self, terms, k=10, frameIds=None, queries=None, what="", **filters):
        """One batched call against the loop of searchFiltered(requiredTerms=) and against the batched call on the model's lists."""
        eng = self.eng
        qs = self.queries[:len(terms)] if queries is None else queries
        nq = len(qs)
        lists = [None] * nq if frameIds is None else frameIds
        got = eng.searchBatchTerms(qs, k, terms, frameIds=frameIds, **filters)

        def per(name, q):
            v = filters.get(name)
            return v[q] if isinstance(v, list) else v
        for q in range(nq):
            kw = {"timeRange": per("timeRange", q), "denyFlags": per("denyFlags", q) or 0, "minScore": per("minScore", q)}
            e_ids, e_scores = eng.searchFiltered(qs[q], k, frameIds=lists[q], requiredTerms=terms[q], **kw)
            c = int(got[2][q])
            assert c == len(e_ids), (what, q, c, len(e_ids))
            assert np.array_equal(got[0][q, :c], e_ids) and np.array_equal(got[1][q, :c].view(np.int32), e_scores.view(np.int32)), (what, q)
        allow = [self.model_ids(terms[q], lists[q]) if terms[q] is not None else lists[q] for q in range(nq)]
        exp = eng.searchBatchFiltered(qs, k, frameIds=allow, **filters)
        assert np.array_equal(got[2], exp[2]), what
        for q in range(nq):
            c = int(got[2][q])
            assert np.array_equal(got[0][q, :c], exp[0][q, :c]) and np.array_equal(got[1][q, :c].view(np.int32), exp[1][q, :c].view(np.int32)), (what, q)
        return got


@pytest.fixture(scope="module")
def stores(wax):
    made = {}

    def get(metric, n):
        if (metric, n) not in made:
            made[(metric, n)] = Store(wax, metric, n, seed=n + len(metric))
        return made[(metric, n)]
    yield get
    for s in made.values():
        s.eng.close()


def delta(eng, before):
    after = eng.termBatchStats()
    return {k: after[k] - before[k] for k in after}


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n", (257, 4097, 9999))
def test_batch_equals_the_loop_and_the_model_lists(stores, n, metric):
    s = stores(metric, n)
    eng = s.eng
    ses = lambda i: [SESSION0 + i]                                  # noqa: E731
    # term and no-term queries; equal sets in another order (and with a duplicate) share one set; a set nothing passes
    terms = [ses(0), None, [TAG0 + 1, SESSION0 + 1], [SESSION0 + 1, TAG0 + 1, SESSION0 + 1], ses(0), [NOBODY], [EVERYBODY, TAG0 + 12], None]
    b0 = eng.termBatchStats()
    got = s.check(terms, what="mixed")
    d = delta(eng, b0)
    assert d == {"calls": 1, "queries": 6, "sets": 4, "mask_launches": 1, "looped": 0, "host_decided": 0}, d
    for q, t in enumerate(terms):                                   # (no other filter: the count is the model's)
        assert got[2][q] == min(10, int(ref.pass_set(s.sets, t).sum()) if t is not None else n), q
    assert got[2][5] == 0 and got[2][0] > 0 and got[2][6] > 0
    # with a predicate, a cut, a short list, a list above 16 384 ids (which loops), all in one call
    short = s.fids[::3][:700]
    long_list = np.concatenate([s.fids[::2], np.arange(2**40, 2**40 + 17_000, dtype=np.uint64)])
    assert len(long_list) > 16_384
    terms = [ses(1), ses(1), ses(2), ses(2), [EVERYBODY, TAG0], ses(3), None, [TAG0 + 2]]
    lists = [None, short, short, long_list, None, None, short, long_list]
    ranges = [(20, 80), None, (None, 50), None, None, (10, None), (20, 80), None]
    denies = [0, 0x100, 0, 0x100, 0x100, 0, 0, 0]
    ref_scores = eng.searchFiltered(s.queries[4], 10, requiredTerms=terms[4], denyFlags=0x100)[1]
    cuts = [None, None, None, None, float(ref_scores[4]), None, None, None]
    b0, t0 = eng.termBatchStats(), eng.termStats()
    got = s.check(terms, frameIds=lists, timeRange=ranges, denyFlags=denies, minScore=cuts, what="combined")
    d = delta(eng, b0)
    assert d["calls"] == 1 and d["looped"] == 2 and d["queries"] == 5 and d["mask_launches"] == 1 and d["sets"] == 4, d
    assert got[2][4] >= 5                                           # the cut is the fifth score of that query
    # k beyond the passing rows, k = 1, and a k above the fused selection (every query takes the single-query body)
    s.check([ses(4), ses(5), None], k=1, what="k=1")
    few = s.check([[SESSION0 + 4, TAG0], [SESSION0 + 5, TAG0 + 1], [SESSION0 + 4, TAG0, TAG0 + 10]], k=150, what="k=150")
    assert (few[2] < 150).all()                                     # fewer passing rows than k: all of them, in order
    b0 = eng.termBatchStats()
    s.check([ses(6), None, ses(7)], k=300, what="k=300")
    assert delta(eng, b0)["looped"] == 2


def test_thirty_three_sets_take_two_launches(stores):
    s = stores("cosine", 9999)
    terms = [[SESSION0 + i] for i in range(33)]
    qs = np.concatenate([s.queries, s.queries, s.queries])[:33]
    b0 = s.eng.termBatchStats()
    got = s.check(terms, queries=qs, what="33 sets")
    d = delta(s.eng, b0)
    assert d["sets"] == 33 and d["mask_launches"] == 2 and d["queries"] == 33 and d["looped"] == 0, d
    assert (got[2] == 10).all()
    # 32 of them: one launch
    b0 = s.eng.termBatchStats()
    s.check(terms[:32], queries=qs[:32], what="32 sets")
    assert delta(s.eng, b0)["mask_launches"] == 1


def test_budget_loops_an_entry_and_counts_it(stores):
    s = stores("cosine", 4097)
    eng = s.eng
    terms = [[SESSION0], [SESSION0 + 1], [EVERYBODY], [SESSION0 + 2]]
    sizes = [int(ref.pass_set(s.sets, t).sum()) for t in terms]
    assert sizes[2] == s.n and max(sizes[0], sizes[1], sizes[3]) < 400
    old = eng.getTuning("predicate_batch_rows")
    try:
        # the upper bound of a term entry is its set's count: three sessions fit 1 000 slots, EVERYBODY (every row) does not
        eng.setTuning("predicate_batch_rows", 1000)
        b0, f0 = eng.termBatchStats(), eng.getTuning("filter_batch_fallbacks")
        s.check(terms, what="budget 1000")
        d = delta(eng, b0)
        assert d["looped"] == 1 and d["queries"] == 3 and d["mask_launches"] == 1 and d["sets"] == 4, d
        assert eng.getTuning("filter_batch_fallbacks") == f0 + 1
        # a budget below the first entry's count loops it and admits the smaller ones behind it
        eng.setTuning("predicate_batch_rows", max(sizes[1], sizes[3]))
        b0 = eng.termBatchStats()
        s.check(terms, what="budget of one session")
        d = delta(eng, b0)
        assert d["looped"] >= 2 and d["looped"] + d["queries"] == 4, d
    finally:
        eng.setTuning("predicate_batch_rows", old)


def test_none_is_the_call_as_it_was(stores):
    """requiredTerms=None (and the C call with both term arrays NULL): the answers, every counter and every read-out of
    searchBatchFiltered without the argument."""
    s = stores("cosine", 4097)
    eng = s.eng
    qs = s.queries[:6]
    lists = [None, s.fids[:300], None, s.fids[::5], None, s.fids[:300]]
    ranges = [(20, 80), None, None, (None, 50), (20, 80), None]
    keys = ("predicate_searches", "predicate_batch_queries", "predicate_batch_classes", "filter_batch_queries", "filter_batch_fallbacks",
            "filter_device_searches", "predicate_gather_searches", "predicate_masked_scans")

    def run(with_terms_none=False):
        before = {k: eng.getTuning(k) for k in keys}
        st0, tb0, tm0 = eng.stats(), eng.termBatchStats(), eng.termStats()
        call = eng.searchBatchTerms if with_terms_none else eng.searchBatchFiltered
        out = call(qs, 10, *((None,) if with_terms_none else ()), frameIds=lists, timeRange=ranges)
        st1 = eng.stats()
        moved = {k: eng.getTuning(k) - v for k, v in before.items()}
        moved["st_searches"] = st1.searches - st0.searches
        moved["st_rows"] = st1.rows_scanned - st0.rows_scanned
        moved["st_bytes"] = st1.bytes_scanned - st0.bytes_scanned
        assert eng.termBatchStats() == tb0 and eng.termStats() == tm0
        return out, moved
    a, moved_a = run()
    b, moved_b = run(with_terms_none=True)
    assert moved_a == moved_b and moved_a["st_searches"] > 0
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # the C call with NULL term arrays, and with arrays whose every length is 0
    nq = len(qs)
    flat, begin, length = s.wax.engine.pack_allow_lists(lists, nq)
    from wax_amd.engine import _row_predicates
    preds = _row_predicates(ranges, [0] * nq)
    u64, u32, f32 = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_float)
    for tb, tl in ((None, None), (np.zeros(nq, dtype=np.uint64), np.zeros(nq, dtype=np.uint32))):
        ids, scores, counts = np.zeros_like(a[0]), np.zeros_like(a[1]), np.zeros_like(a[2])
        tb0 = eng.termBatchStats()
        rc = eng._lib.wax_hip_search_batch_terms(
            eng._h, np.ascontiguousarray(qs).ctypes.data_as(f32), nq, DIMS, 10, flat.ctypes.data_as(u64), int(flat.size), begin.ctypes.data_as(u64),
            length.ctypes.data_as(u64), None, preds, None, 0, None if tb is None else tb.ctypes.data_as(u64),
            None if tl is None else tl.ctypes.data_as(u32), ids.ctypes.data_as(u64), scores.ctypes.data_as(f32), ids.shape[1], counts.ctypes.data_as(u32))
        assert rc == 0 and eng.termBatchStats() == tb0
        assert np.array_equal(ids, a[0]) and np.array_equal(scores, a[1]) and np.array_equal(counts, a[2])


def test_refusals_leave_the_outputs_and_name_the_query(stores):
    from wax_amd import _abi
    s = stores("cosine", 257)
    eng = s.eng
    nq = 3
    qs = np.ascontiguousarray(s.queries[:nq])
    u64, u32, f32 = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_float)
    terms = np.arange(40, dtype=np.uint32)

    def call(begin, length, n_terms=40, dims=DIMS, terms_ptr=terms.ctypes.data_as(u32)):
        ids, scores, counts = np.full((nq, 10), 5, dtype=np.uint64), np.full((nq, 10), 2, dtype=np.float32), np.full(nq, 77, dtype=np.uint32)
        b = None if begin is None else np.array(begin, dtype=np.uint64)
        ln = None if length is None else np.array(length, dtype=np.uint32)
        rc = eng._lib.wax_hip_search_batch_terms(eng._h, qs.ctypes.data_as(f32), nq, dims, 10, None, 0, None, None, None, None, terms_ptr, n_terms,
                                                 None if b is None else b.ctypes.data_as(u64), None if ln is None else ln.ctypes.data_as(u32),
                                                 ids.ctypes.data_as(u64), scores.ctypes.data_as(f32), 10, counts.ctypes.data_as(u32))
        untouched = bool((ids == 5).all() and (scores == 2).all() and (counts == 77).all())
        return rc, _abi.last_error(), untouched
    b0 = eng.termBatchStats()
    rc, msg, same = call([0, 1, 2], None)
    assert rc == _abi.ERR_INVALID_ARGUMENT and "both" in msg and same
    rc, msg, same = call(None, [1, 1, 1])
    assert rc == _abi.ERR_INVALID_ARGUMENT and "both" in msg and same
    for begin, length in (([0, 0, 39], [1, 1, 2]), ([0, 41, 0], [1, 0, 1]), ([0, 0, 2**63], [1, 1, 2])):
        rc, msg, same = call(begin, length)
        q = 2 if begin[2] else 1
        assert rc == _abi.ERR_INVALID_ARGUMENT and "leaves the term array" in msg and f"query {q}" in msg and same, (begin, length, msg)
    rc, msg, same = call([0, 0, 0], [1, 17, 1])
    assert rc == _abi.ERR_INVALID_ARGUMENT and "more than 16" in msg and "query 1" in msg and same
    rc, msg, same = call([0, 0, 0], [1, 1, 1], terms_ptr=None)
    assert rc == _abi.ERR_INVALID_ARGUMENT and same
    rc, msg, same = call([0, 0, 0], [1, 1, 1], dims=DIMS - 1)      # the batched predicate search's own refusals come first
    assert rc == _abi.ERR_DIM_MISMATCH and same
    rc, msg, same = call([0, 41, 0], [1, 0, 1], dims=DIMS - 1)
    assert rc == _abi.ERR_DIM_MISMATCH and same
    assert eng.termBatchStats() == b0
    # 40 entries of 16 distinct terms are fine: duplicates collapse first
    dup = np.array(list(range(16)) * 2 + [3] * 8, dtype=np.uint32)
    rc, msg, same = call([0, 0, 0], [40, 0, 16], terms_ptr=dup.ctypes.data_as(u32))
    assert rc == 0 and not same


def test_a_store_without_terms_answers_empty_on_the_host(wax):
    s = Store(wax, "cosine", 600, seed=77, terms=False)
    eng = s.eng
    try:
        terms = [[EVERYBODY], None, [SESSION0, TAG0], None]
        b0, m0 = eng.termBatchStats(), eng.termStats()
        got = s.check(terms, frameIds=[None, None, s.fids[:100], s.fids[:100]], what="no terms")
        d = delta(eng, b0)
        assert d["host_decided"] == 2 and d["mask_launches"] == 0 and d["queries"] == 0 and d["sets"] == 0 and d["looped"] == 0, d
        assert got[2].tolist() == [0, 10, 0, 10]
        m1 = eng.termStats()
        assert m1["term_rows_uploaded"] == m0["term_rows_uploaded"] == 0 and m1["device_masks"] == 0
        assert eng.searchBatchTerms(s.queries[:2], 10, wax.TermDictionary.NO_MATCH)[2].tolist() == [0, 0]
        mixed = eng.searchBatchTerms(s.queries[:2], 10, [wax.TermDictionary.NO_MATCH, None])
        assert mixed[2].tolist() == [0, 10] and np.array_equal(mixed[0][1], eng.searchBatch(s.queries[1:2], 10)[0][0])
    finally:
        eng.close()


def test_after_mutations_against_a_rebuilt_store(wax):
    """remove, removeBatch and setTerms on one store; a second store built from what is left: the same batched answers."""
    n = 3000
    s = Store(wax, "cosine", n, seed=91)
    model = ref.StoreModel(DIMS)
    model.add_batch(s.fids, s.rows)
    model.set_terms(s.fids, s.sets)
    eng = s.eng
    terms = [[SESSION0], [SESSION0 + 1, TAG0 + 1], None, [EVERYBODY, TAG0 + 12], [SESSION0 + 2], [SESSION0]]
    lists = [None, None, None, None, s.fids[::4], s.fids[::4]]
    qs = s.queries[:6]

    def same(what):
        fids = np.asarray(model.ids, dtype=np.uint64)
        rebuilt = wax.HIPVectorEngine(metric=wax.VectorMetric.cosine, dimensions=DIMS)
        try:
            rebuilt.addBatch(fids, model.matrix())
            rebuilt.setTerms(fids, model.sets)
            a = eng.searchBatchTerms(qs, 10, terms, frameIds=lists)
            b = rebuilt.searchBatchTerms(qs, 10, terms, frameIds=lists)
            assert np.array_equal(a[2], b[2]) and (a[2] > 0).all(), what
            for q in range(len(qs)):
                c = int(a[2][q])
                assert np.array_equal(a[0][q, :c], b[0][q, :c]) and np.array_equal(a[1][q, :c].view(np.int32), b[1][q, :c].view(np.int32)), (what, q)
                e_ids, e_scores = eng.searchFiltered(qs[q], 10, frameIds=lists[q], requiredTerms=terms[q])
                assert np.array_equal(a[0][q, :c], e_ids) and np.array_equal(a[1][q, :c], e_scores), (what, q)
                want = model.passing_ids(terms[q]) if terms[q] is not None else fids
                assert np.isin(a[0][q, :c], want).all(), (what, q)
        finally:
            rebuilt.close()
    same("as built")
    first = eng.searchBatchTerms(qs[:1], 10, [terms[0]])
    eng.remove(int(first[0][0, 0])); model.remove(int(first[0][0, 0]))
    same("remove of the best hit")
    gone = s.fids[[7, 300, 301, 1599, n - 1]]
    assert eng.removeBatch(gone) == len([g for g in gone if int(g) in model.ids])
    model.remove_batch(gone)
    same("removeBatch")
    u0 = eng.termStats()["term_rows_uploaded"]
    moved = s.fids[100:140]
    new_sets = [(SESSION0, TAG0 + 1, EVERYBODY)] * 20 + [()] * 20
    eng.setTerms(moved, new_sets); model.set_terms(moved, new_sets)
    same("setTerms")
    assert eng.termStats()["term_rows_uploaded"] > u0                # the batched pass uploaded the changed rows (ensure_terms)
    eng.close()


def test_three_shards_answer_as_one_engine(wax):
    n = 3000
    one = Store(wax, "cosine", n, seed=41)
    many = Store(wax, "cosine", n, seed=41, devices=[0, 0, 0])
    try:
        assert many.eng.shardCount == 3 and all(many.eng.shardInfo(g)[2] > 0 for g in range(3))
        terms = [[SESSION0], None, [SESSION0 + 1, TAG0 + 1], [NOBODY], [EVERYBODY, TAG0 + 12], [SESSION0]]
        lists = [None, None, None, None, one.fids[::3], one.fids[:20000:2]]
        ranges = [(20, 80), None, None, None, None, None]
        b0 = many.eng.termBatchStats()
        a = one.check(terms, frameIds=lists, timeRange=ranges, what="one engine")
        b = many.check(terms, frameIds=lists, timeRange=ranges, what="three shards")
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        d = delta(many.eng, b0)
        assert d["calls"] >= 3 and d["mask_launches"] == 3 and d["queries"] == 3 * 5, d     # every shard ran its own pass (check() calls once with terms)
    finally:
        one.eng.close()
        many.eng.close()
