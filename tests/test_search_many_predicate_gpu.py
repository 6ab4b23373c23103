"""One query each against many small stores with a row predicate and a score cut per pair (wax_hip_search_many_predicate /
wax_amd.searchManyFiltered): row i must equal what engines[i].searchFiltered(queries[i], topK, timeRange=, denyFlags=, minScore=)
returns — ids, scores and counts bit for bit — whether a masked group of the pooled launch, an unmasked one or the single-query
predicate search answered the pair, and the read-only counters must show which did."""
import ctypes

import numpy as np
import pytest

import oracle
from helpers import assert_parity

pytestmark = pytest.mark.gpu

GROUP = {64: 16, 384: 32, 768: 64}     # row_math.h's lane-shape table at the dims under test
N_ENGINES = 24
KS = (1, 10, 60, 61, 192, 193)         # 61: 256-slot lists where LDS allows; 193: always the loop
DUP, SEVENTEEN, APPENDED = 11, 10, 23  # the duplicated 3 000-row store (listed 33 times), the store listed 17 times, attributes then 50 appended rows
NO_ATTRS = (17, 22)                    # never get attributes (32 and 16 * rpc + 3 rows)
TS0 = 1000                             # timestamp of row 0; they ascend with the row


@pytest.fixture(scope="module")
def wax(hip_lib):
    import wax_amd
    if hip_lib.wax_hip_device_count() == 0:
        pytest.skip("no HIP device on this host: the gpu-marked tests run on the MI355X box (pytest -m gpu)")
    assert hip_lib.wax_hip_available() == 1, "a HIP device is visible but it is not gfx950: the HIP path needs an MI355X"
    return wax_amd


def rpc(dims):
    """rows a wave consumes per chunk"""
    return (64 // GROUP[dims]) * 4


def pooled_shape(dims, k):
    """scan_multi_group(dims, k) != 0: k <= 192 and the 16 queries with their four wave lists (64 slots while k + 4 <= 64, else 256)
    fit the 160 KB of LDS (multiscan.hip: scan_multi_lds_bytes)."""
    if k < 1 or k > 192:
        return False
    cap = 64 if k + 4 <= 64 else 256
    return 16 * dims * 4 + 4 * 16 * cap * 8 + 4 * 16 * 16 + 16 * 4 + 16 * 4 * 4 + 16 <= 160 * 1024


def corpus_for(metric, n, dims, seed):
    x = oracle.gaussian_unit_rows(seed * 100003, n, dims)
    if metric == 1:   # dot: rows of different norms
        x = x * np.random.default_rng(seed + 7).uniform(0.5, 2.0, size=(n, 1)).astype(np.float32)
    return np.ascontiguousarray(x, dtype=np.float32)


def make_engine(wax, metric, dims, corpus=None, ids=None, **kw):
    eng = wax.HIPVectorEngine(metric=wax.VectorMetric(metric), dimensions=dims, **kw)
    if corpus is not None and len(corpus):
        eng.addBatch(ids, corpus)
    return eng


def is_empty(tr, deny):
    return (tr is None or (tr[0] is None and tr[1] is None)) and not deny


def passes(tr, deny, ts, flags):
    """the predicate on numpy columns"""
    ok = (flags & np.uint32(deny)) == 0
    if tr is not None and tr[0] is not None:
        ok &= ts >= tr[0]
    if tr is not None and tr[1] is not None:
        ok &= ts < tr[1]
    return ok


def norm_key(tr, deny):
    """what two pairs must share to share a pass"""
    return (None if tr is None else tr[0], None if tr is None else tr[1], int(deny))


def loop(pairs, queries, k, ranges, denies, cuts):
    return [pairs[i].searchFiltered(queries[i], k, timeRange=ranges[i], denyFlags=denies[i], minScore=cuts[i]) for i in range(len(pairs))]


def assert_rows_equal(many, ref, ctx):
    ids, scores, counts = many
    for i, (ri, rs) in enumerate(ref):
        n = int(counts[i])
        assert n == len(ri), f"{ctx}: pair {i} count {n} != {len(ri)}"
        assert np.array_equal(ids[i, :n], ri), f"{ctx}: pair {i} ids"
        assert np.array_equal(scores[i, :n], rs), f"{ctx}: pair {i} scores"


ROUTE_KEYS = ("search_many_pooled", "search_many_looped", "search_many_masked")


def counters(engines):
    distinct = {id(e): e for e in engines}.values()
    return {id(e): tuple(e.getTuning(k) for k in ROUTE_KEYS) for e in distinct}


def assert_route(engines, before, pooled, masked_pairs, ctx):
    """every pair went the expected way: per distinct engine, the counter of its route grew by its pairs and the other stood still;
    "search_many_masked" grew by masked_pairs(e) where the engine was pooled and stood still where it looped"""
    after = counters(engines)
    for e in {id(e): e for e in engines}.values():
        pairs = sum(1 for x in engines if x is e)
        d = tuple(a - b for a, b in zip(after[id(e)], before[id(e)]))
        want = pooled(e) if callable(pooled) else pooled
        exp = (pairs, 0, masked_pairs(e)) if want else (0, pairs, 0)
        assert d == exp, f"{ctx}: engine of {e.count} rows listed {pairs}x: pooled / looped / masked +{d}, expected +{exp}"


class Stores:
    """24 engines of one (dims, metric), sizes around the chunk and the bitmap word, overlapping id spaces, attributes on most; a
    list of 100 pairs, each with its predicate and (a third of them) its score cut."""

    def __init__(self, wax, dims, metric):
        r = rpc(dims)
        sizes = [0, r - 1, r, r + 1, 31, 32, 33, 63, 64, 65, 16 * r + 3, 3000]
        rng = np.random.default_rng(dims * 10 + metric + 1)
        self.dims, self.metric = dims, metric
        self.engines, self.corpora, self.ids, self.ts, self.flags = [], [], [], [], []
        for j in range(N_ENGINES):
            n = sizes[j % len(sizes)]
            extra = 50 if j == APPENDED else 0
            c = corpus_for(metric, n + extra, dims, seed=j + 1)
            if j == DUP:   # exactly duplicated rows (the tie order is ascending ROW, not ascending id)
                c[100:110] = c[50]
                c[2990:2995] = c[50]
            ids = (1000 * j + rng.permutation(n + extra)).astype(np.uint64)   # engine j's ids overlap its neighbours'; row order != id order
            eng = make_engine(wax, metric, dims, c[:n], ids[:n])
            ts, fl = np.zeros(n + extra, np.int64), np.zeros(n + extra, np.uint32)
            if n and j not in NO_ATTRS:
                ts[:n] = TS0 + np.arange(n)
                bits = rng.random((n, 4)) < 0.2
                fl[:n] = (bits[:, 0] * 1 + bits[:, 1] * 2 + bits[:, 2] * 4 + bits[:, 3] * 256).astype(np.uint32)
                if j == DUP:   # a deny flag on SOME of the duplicates
                    fl[[50] + list(range(105, 110)) + list(range(2990, 2995))] = 0
                    fl[100:105] = 1
                assert eng.setAttributes(ids[:n], ts[:n], fl[:n]) == n
            if extra:          # appended after the attributes were set: the new rows read (0, 0)
                eng.addBatch(ids[n:], c[n:])
            self.engines.append(eng)
            self.corpora.append(c)
            self.ids.append(ids)
            self.ts.append(ts)
            self.flags.append(fl)
        order = [SEVENTEEN] * 17 + [DUP] * 33 + [0] * 2           # 17 and 33 pairs of one engine; the empty engine twice
        rest = [j for j in range(N_ENGINES) if j not in (0, SEVENTEEN, DUP)]
        order += rest + rest + [APPENDED] * 6
        assert len(order) == 100
        self.order = [int(j) for j in rng.permutation(order)]
        self.queries = oracle.gaussian_unit_queries(100, dims, seed=dims + metric).copy()
        self.ranges, self.denies, self.cuts = [], [], []
        cut_values = [float("nan"), 0.1, -1.35, 0.2, -0.5]
        seen_dup = 0
        for i, j in enumerate(self.order):
            n = self.engines[j].count
            if j == DUP and i % 2 == 0:   # half of the duplicated store's queries sit on its duplicated row: the ties are the top hits
                self.queries[i] = self.corpora[DUP][50] + 1e-3 * self.queries[i]
            quarter = (TS0 + n // 4, TS0 + n // 2)
            kinds = [(None, 0),                                  # no predicate
                     (None, 0b111),                              # the default FrameFilter()
                     (quarter, 0),                               # a contiguous quarter: whole chunks are clear
                     ((int(self.ts[j].max()) if n else TS0, None), 0),   # exactly the last row with a timestamp
                     ((10**9, None), 0),                         # nothing
                     ((-5, None), 0),                            # a non-empty predicate every row passes, (0, 0) included
                     ((TS0, TS0 + 3), 0x100),                    # fewer rows than k
                     ((None, TS0 + n // 2), 0b10)]
            if j == DUP:   # three predicates interleaved: its 33 queries split into three classes of 11
                tr, deny = [kinds[1], kinds[2], kinds[5]][seen_dup % 3]
                seen_dup += 1
            else:
                tr, deny = kinds[i % len(kinds)]
            self.ranges.append(tr)
            self.denies.append(deny)
            self.cuts.append(cut_values[(i // 3) % len(cut_values)] if i % 3 == 0 else None)
        self.pairs = [self.engines[j] for j in self.order]
        self.ref = {}

    def reference(self, k):
        if k not in self.ref:
            self.ref[k] = loop(self.pairs, self.queries, k, self.ranges, self.denies, self.cuts)
        return self.ref[k]

    def many(self, wax, k):
        return wax.searchManyFiltered(self.pairs, self.queries, k, timeRange=self.ranges, denyFlags=self.denies, minScore=self.cuts)

    def masked_pairs(self, e):
        """pairs of engine e a masked group answers when e is pooled: a non-empty predicate on a store with rows and attributes"""
        j = next(x for x in range(N_ENGINES) if self.engines[x] is e)
        if e.count == 0 or j in NO_ATTRS:
            return 0
        return sum(1 for i, x in enumerate(self.order) if x == j and not is_empty(self.ranges[i], self.denies[i]))

    def groups(self, e):
        """passes over engine e's store when it is pooled: per class of pairs that share a predicate, one per 16"""
        j = next(x for x in range(N_ENGINES) if self.engines[x] is e)
        if e.count == 0:
            return 0
        classes = {}
        for i, x in enumerate(self.order):
            if x != j:
                continue
            tr, deny = self.ranges[i], self.denies[i]
            key = norm_key(None, 0) if is_empty(tr, deny) else norm_key(tr, deny)
            if j in NO_ATTRS and not is_empty(tr, deny):
                if not passes(tr, deny, np.zeros(1, np.int64), np.zeros(1, np.uint32))[0]:
                    continue                          # decided on the host: count 0, no pass
                key = norm_key(None, 0)               # every row passes: an unmasked pair
            classes[key] = classes.get(key, 0) + 1
        return sum((c + 15) // 16 for c in classes.values())

    def close(self):
        for e in self.engines:
            e.close()


@pytest.fixture(scope="module")
def stores(wax):
    made = {}

    def get(dims, metric):
        if (dims, metric) not in made:
            made[(dims, metric)] = Stores(wax, dims, metric)
        return made[(dims, metric)]
    yield get
    for s in made.values():
        s.close()


@pytest.mark.parametrize("metric", [0, 1, 2], ids=["cosine", "dot", "l2"])
@pytest.mark.parametrize("dims", [64, 384, 768])
def test_equals_the_single_store_call(wax, stores, dims, metric):
    s = stores(dims, metric)
    assert s.engines[APPENDED].count == 3050 and s.engines[SEVENTEEN].count == 16 * rpc(dims) + 3
    for k in KS:
        ref = s.reference(k)
        before = counters(s.pairs)
        got = s.many(wax, k)
        assert_rows_equal(got, ref, f"dims {dims} metric {metric} k {k}")
        assert_route(s.pairs, before, pooled_shape(dims, k), s.masked_pairs, f"dims {dims} metric {metric} k {k}")
    assert pooled_shape(dims, 60) and not pooled_shape(dims, 193)
    assert pooled_shape(dims, 61) == (dims < 768)      # 256-slot lists beside sixteen 768-d queries do not fit LDS
    # the cases are what they claim to be: some pairs come back short, some empty, some cut by minScore
    counts = s.many(wax, 10)[2]
    assert (counts == 0).any() and ((counts > 0) & (counts < 10)).any() and (counts == 10).any()
    assert s.masked_pairs(s.engines[DUP]) == 33 and s.groups(s.engines[DUP]) == 3


def test_against_the_oracle(wax, stores):
    """The answer is independent of the device path: the oracle on the rows a numpy mask lets pass."""
    s, k = stores(384, 0), 10
    ids, scores, counts = wax.searchManyFiltered(s.pairs, s.queries, k, timeRange=s.ranges, denyFlags=s.denies)
    checked = 0
    for i, j in enumerate(s.order):
        n = s.engines[j].count
        if n == 0:
            assert counts[i] == 0
            continue
        mask = passes(s.ranges[i], s.denies[i], s.ts[j][:n], s.flags[j][:n])
        c = int(counts[i])
        assert c == min(k, int(mask.sum())), f"pair {i}: {c} results, {int(mask.sum())} rows pass"
        if c == 0:
            continue
        rows, rid = s.corpora[j][:n][mask], s.ids[j][:n][mask]
        ei, es, _, _ = oracle.search(0, rows, rid, s.queries[i], k)
        _, es_all, _, _ = oracle.search(0, rows, rid, s.queries[i], 2 * k)
        assert_parity(ids[i, :c], scores[i, :c], ei, es, all_exp_scores=es_all, ctx=f"pair {i} (engine {j})")
        checked += 1
    assert checked >= 60


def test_ties_come_in_ascending_row_order(wax, stores):
    s = stores(384, 0)
    e, ids = s.engines[DUP], s.ids[DUP]
    q = np.stack([s.corpora[DUP][50]] * 2)
    before = counters([e])
    got_ids, _, counts = wax.searchManyFiltered([e, e], q, 11, denyFlags=0b111)
    want = [int(ids[r]) for r in [50] + list(range(105, 110)) + list(range(2990, 2995))]    # rows 100..104 carry the deleted bit
    assert counts.tolist() == [11, 11] and got_ids[0].tolist() == want and got_ids[1].tolist() == want
    assert_route([e, e], before, True, lambda _: 2, "ties")


def test_without_filters_it_is_search_many(wax, stores):
    s = stores(384, 0)

    def run(fn):
        c0 = counters(s.pairs)
        st0 = {id(e): e.stats() for e in s.engines}
        out = fn()
        c1 = counters(s.pairs)
        st1 = {id(e): e.stats() for e in s.engines}
        return out, ({i: tuple(a - b for a, b in zip(c1[i], c0[i])) for i in c0},
                     {i: (st1[i].searches - st0[i].searches, st1[i].rows_scanned - st0[i].rows_scanned,
                          st1[i].bytes_scanned - st0[i].bytes_scanned) for i in st0})
    for k in (10, 193):
        want, dw = run(lambda: wax.searchMany(s.pairs, s.queries, k))
        got, dg = run(lambda: wax.searchManyFiltered(s.pairs, s.queries, k))
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), f"k {k}"
        assert dg == dw, f"k {k}"
        got, dg = run(lambda: wax.searchManyFiltered(s.pairs, s.queries, k, timeRange=[(None, None)] * 100, denyFlags=[0] * 100,
                                                            minScore=[float("nan")] * 100))      # arrays of empty predicates and NaN cuts
        assert all(np.array_equal(a, b) for a, b in zip(got, want)) and dg == dw, f"k {k}, per-pair empties"


def test_stores_without_attributes(wax, stores):
    s = stores(384, 0)
    engines = [s.engines[j] for j in NO_ATTRS] * 2
    queries = oracle.gaussian_unit_queries(4, 384, seed=21)
    plain = wax.searchMany(engines, queries, 10)
    before = counters(engines)
    got = wax.searchManyFiltered(engines, queries, 10, timeRange=(None, 5), denyFlags=0b111)     # (0, 0) passes: the unmasked answer
    assert all(np.array_equal(a, b) for a, b in zip(got, plain)) and (got[2] > 0).all()
    assert_route(engines, before, True, lambda _: 0, "(0, 0) passes")
    before = counters(engines)
    ids, scores, counts = wax.searchManyFiltered(engines, queries, 10, timeRange=(5, None))      # (0, 0) fails: nothing, and no device work
    assert counts.tolist() == [0, 0, 0, 0]
    assert_route(engines, before, True, lambda _: 0, "(0, 0) fails")
    for e in engines:
        assert e.getTuning("attr_device_rows") == 0
        assert e.searchFiltered(queries[0], 10, timeRange=(5, None))[0].size == 0


def test_attributes_set_just_before_the_call_are_seen(wax):
    dims = 384
    corpora = [corpus_for(0, 200, dims, seed=40 + j) for j in range(3)]
    engines = [make_engine(wax, 0, dims, corpora[j], (1000 * j + np.arange(200)).astype(np.uint64)) for j in range(3)]
    queries = oracle.gaussian_unit_queries(3, dims, seed=5).copy()
    for j, e in enumerate(engines):
        e.setAttributes((1000 * j + np.arange(200)).astype(np.uint64), np.arange(200, dtype=np.int64) + 10, np.zeros(200, np.uint32))
    first = wax.searchManyFiltered(engines, queries, 5, timeRange=(None, 10**6), denyFlags=1)
    best = [int(first[0][j, 0]) for j in range(3)]
    engines[0].setAttributes([best[0]], None, [1])               # the best hit is deleted just before the call
    engines[1].add(999_999, queries[1])                           # staged on the host until the next reader flushes it; it reads (0, 0)
    engines[2].setAttributes([best[2]], [10**7], None)            # moved out of the time range
    before = counters(engines)
    ids, scores, counts = wax.searchManyFiltered(engines, queries, 5, timeRange=(None, 10**6), denyFlags=1)
    assert_route(engines, before, True, lambda _: 1, "fresh attributes")
    assert best[0] not in ids[0].tolist() and best[2] not in ids[2].tolist()
    assert ids[1, 0] == 999_999 and abs(float(scores[1, 0]) - 1.0) < 1e-5
    assert_rows_equal((ids, scores, counts), loop(engines, queries, 5, [(None, 10**6)] * 3, [1] * 3, [None] * 3), "fresh attributes")
    for e in engines:
        e.close()


def test_switches_route_per_engine(wax, stores):
    s = stores(384, 0)
    ref = s.reference(10)
    big = lambda e: e.count > 1000
    try:
        for e in s.engines:
            e.setTuning("search_many_max_rows", 1000)
        before = counters(s.pairs)
        assert_rows_equal(s.many(wax, 10), ref, "max_rows 1000")
        assert any(big(e) for e in s.pairs) and not all(big(e) for e in s.pairs)
        assert_route(s.pairs, before, lambda e: not big(e), s.masked_pairs, "max_rows 1000")      # looped and pooled pairs in ONE call
    finally:
        for e in s.engines:
            e.setTuning("search_many_max_rows", 262144)
    for key, on, off_value in (("search_many", 1, 0), ("force_general", 0, 1)):
        off = s.engines[SEVENTEEN]
        try:
            off.setTuning(key, off_value)
            before = counters(s.pairs)
            assert_rows_equal(s.many(wax, 10), ref, f"{key} {off_value} on one engine")
            assert_route(s.pairs, before, lambda e: e is not off, s.masked_pairs, f"{key} {off_value} on one engine")
        finally:
            off.setTuning(key, on)
    try:
        for e in s.engines:
            e.setTuning("search_many", 0)
        before = counters(s.pairs)
        assert_rows_equal(s.many(wax, 10), ref, "search_many 0")
        assert_route(s.pairs, before, False, s.masked_pairs, "search_many 0")
    finally:
        for e in s.engines:
            e.setTuning("search_many", 1)


def test_accounting(wax, stores):
    s = stores(384, 0)
    seen = {}
    for i, e in enumerate(s.pairs):
        ent = seen.setdefault(id(e), [e, 0, 0])
        ent[1] += 1
        ent[2] += 0 if is_empty(s.ranges[i], s.denies[i]) else 1
    before = {i: (e.stats(), e.getTuning("predicate_searches")) for i, (e, _, _) in seen.items()}
    s.many(wax, 10)
    for i, (e, n, n_pred) in seen.items():
        st0, st1 = before[i][0], e.stats()
        groups = s.groups(e)
        assert st1.searches - st0.searches == n
        assert st1.rows_scanned - st0.rows_scanned == e.count * groups          # the whole store once per group, masked or not
        assert st1.bytes_scanned - st0.bytes_scanned == e.count * groups * 384 * 4
        assert e.getTuning("predicate_searches") - before[i][1] == n_pred


def raw_many(hip_lib, engines, queries, k, stride):
    """the C call itself with a predicate and a cut on every pair, outputs pre-filled with 7: (rc, message, ids, scores, counts)"""
    from wax_amd import _abi
    f32, u32, u64 = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
    n = len(engines)
    handles = (ctypes.c_void_p * n)(*[e._h.value for e in engines])
    q = np.ascontiguousarray(queries, dtype=np.float32)
    preds = (_abi.RowPredicate * n)(*[_abi.RowPredicate(1, 0, 0, 0, 0b111) for _ in range(n)])
    cuts = np.full(n, -1.0, np.float32)
    ids, scores, counts = np.full((n, stride), 7, np.uint64), np.full((n, stride), 7, np.float32), np.full(n, 7, np.uint32)
    rc = hip_lib.wax_hip_search_many_predicate(handles, q.ctypes.data_as(f32), n, q.shape[1], k, preds, cuts.ctypes.data_as(f32),
                                               ids.ctypes.data_as(u64), scores.ctypes.data_as(f32), stride, counts.ctypes.data_as(u32))
    return rc, _abi.last_error(), ids, scores, counts


def test_refusals_touch_nothing(wax, hip_lib):
    from wax_amd import _abi
    dims = 64
    c = corpus_for(0, 50, dims, seed=3)
    ids = np.arange(50, dtype=np.uint64)
    a, b = make_engine(wax, 0, dims, c, ids), make_engine(wax, 0, dims, c, ids)
    other_dims = make_engine(wax, 0, 128, corpus_for(0, 50, 128, seed=3), ids)
    other_metric = make_engine(wax, 2, dims, c, ids)
    sharded = make_engine(wax, 0, dims, c, ids, devices=[0, 0])
    q = oracle.gaussian_unit_queries(3, dims)
    cases = [([a, b, other_dims], _abi.ERR_DIM_MISMATCH, "pair 2"),
             ([a, other_metric, b], _abi.ERR_INVALID_ARGUMENT, "pair 1"),
             ([a, b, sharded], _abi.ERR_INVALID_ARGUMENT, "pair 2")]
    for engines, code, who in cases:
        before = counters([a, b])
        pred_before = [e.getTuning("predicate_searches") for e in (a, b)]
        rc, msg, ids_o, scores_o, counts_o = raw_many(hip_lib, engines, q, 10, 10)
        assert rc == code and who in msg, (rc, msg)
        assert (ids_o == 7).all() and (scores_o == 7).all() and (counts_o == 7).all(), msg
        assert counters([a, b]) == before and [e.getTuning("predicate_searches") for e in (a, b)] == pred_before
    rc, msg, ids_o, _, counts_o = raw_many(hip_lib, [a, b, a], q, 10, 10)      # the same arguments on three good engines are served
    assert rc == _abi.OK and counts_o.tolist() == [10, 10, 10], msg
    with pytest.raises(Exception):
        wax.searchManyFiltered([a, b, sharded], q, 10, denyFlags=1)
    for e in (a, b, other_dims, other_metric, sharded):
        e.close()
