"""Predicate search (wax_hip_search_predicate / searchFiltered(timeRange=, denyFlags=)) and the per-row attributes behind it.

Expected answers. top_k is capped at 10 000, so a full ranking is not available; every answer is checked against
  (a) today's searchFiltered(frameIds = the ids a numpy model of the predicate says pass) on the same engine: ids and scores
      array_equal — the allow-list route scores the same rows with the scan's arithmetic;
  (b) the oracle's f64 ranking of the passing subset, under helpers.assert_parity.
Both routes (gather, masked scan) are forced through "predicate_route" and must agree with (a) and with each other, and the
counters must show which route ran. Shapes: 20 011 x 384 (ragged last chunk, several grid-stride iterations per wave under the
small-store grid rule), 3 001 x 768, 5 003 x 100 (generic dims: gather only)."""
import ctypes

import numpy as np
import pytest

import oracle
from helpers import assert_parity

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
# flag bits of the shared stores: 0 / 1 / 2 as the header names them, bit 8 a random half, 9 all rows but ONE, 10 all rows but the final
# partial chunk's, 11 every row, 12 no row
B_HALF, B_BUT_ONE, B_BUT_TAIL, B_ALL, B_NONE = 1 << 8, 1 << 9, 1 << 10, 1 << 11, 1 << 12
CHUNK = {384: 8, 768: 2}          # rows per chunk of the masked scan


@pytest.fixture(scope="module")
def wax(hip_lib):
    import wax_amd
    if hip_lib.wax_hip_device_count() == 0:
        pytest.skip("no HIP device on this host: the gpu-marked tests run on the MI355X box (pytest -m gpu)")
    assert hip_lib.wax_hip_available() == 1, "a HIP device is visible but it is not gfx950: the HIP path needs an MI355X"
    return wax_amd


def corpus_for(metric, n, dims, seed=0):
    x = oracle.gaussian_unit_rows(seed, n, dims)
    if metric == 1:   # dot: rows of different norms
        x = x * np.random.default_rng(seed + 7).uniform(0.5, 2.0, size=(n, 1)).astype(np.float32)
    return np.ascontiguousarray(x, dtype=np.float32)


class Store:
    """An engine with attributes, and the numpy model of them (row order)."""

    def __init__(self, wax, metric, n, dims, seed, **kw):
        self.metric, self.n, self.dims = metric, n, dims
        self.corpus = corpus_for(metric, n, dims, seed)
        self.ids = (np.arange(n, dtype=np.uint64) * 3 + 7)
        rng = np.random.default_rng(seed + 100)
        self.ts = np.arange(n, dtype=np.int64) - 10_000          # ascending, negative for the first 10 000 rows
        self.ts[0], self.ts[-1] = I64_MIN, I64_MAX
        fl = np.zeros(n, dtype=np.uint32)
        for bit in (0, 1, 2):
            fl[rng.random(n) < 0.1] |= np.uint32(1 << bit)
        fl[rng.random(n) < 0.5] |= np.uint32(B_HALF)
        fl |= np.uint32(B_BUT_ONE | B_BUT_TAIL | B_ALL)
        self.one_row = n // 2 + 3
        fl[self.one_row] &= np.uint32(~B_BUT_ONE & 0xffffffff)
        self.tail0 = n - (n % 8 or 8)                              # first row of the final (partial) 8-row chunk
        fl[self.tail0:] &= np.uint32(~B_BUT_TAIL & 0xffffffff)
        self.fl = fl
        self.eng = wax.HIPVectorEngine(metric=wax.VectorMetric(metric), dimensions=dims, **kw)
        if kw.get("devices"):
            self.eng.setTuning("shard_min_mb", 0)
        self.eng.addBatch(self.ids, self.corpus)
        assert self.eng.setAttributes(self.ids, self.ts, self.fl) == n
        self.queries = oracle.gaussian_unit_queries(8, dims)

    def passing(self, timeRange=None, deny=0, allow=None):
        after, before = (None, None) if timeRange is None else timeRange
        m = (self.fl & np.uint32(deny)) == 0
        if after is not None:
            m &= self.ts >= after
        if before is not None:
            m &= self.ts < before
        if allow is not None:
            m &= np.isin(self.ids, np.asarray(allow, dtype=np.uint64))
        return m


@pytest.fixture(scope="module")
def s384(wax):
    s = Store(wax, 0, 20_011, 384, seed=1)
    yield s
    s.eng.close()


@pytest.fixture(scope="module")
def s768(wax):
    s = Store(wax, 0, 3_001, 768, seed=2)
    yield s
    s.eng.close()


@pytest.fixture(scope="module")
def s100(wax):
    s = Store(wax, 0, 5_003, 100, seed=3)
    yield s
    s.eng.close()


COUNTERS = ("predicate_searches", "predicate_gather_searches", "predicate_masked_scans")


def check(s, k, timeRange=None, deny=0, allow=None, minScore=None, q=0, parity=True, dropped=0, ctx=""):
    """Both routes against (a) and (b); returns the passing-row mask. `dropped`: passing rows whose distance is not finite."""
    eng, query = s.eng, s.queries[q]
    mask = s.passing(timeRange, deny, allow)
    m = int(mask.sum())
    ref = eng.searchFiltered(query, k, frameIds=s.ids[mask], minScore=minScore)                         # (a)
    scan_ok = s.dims in CHUNK and min(max(k, 1), 10_000) <= 192
    for route in (1, 2):
        eng.setTuning("predicate_route", route)
        before = [eng.getTuning(c) for c in COUNTERS]
        got = eng.searchFiltered(query, k, frameIds=allow, minScore=minScore, timeRange=timeRange, denyFlags=deny)
        delta = [eng.getTuning(c) - b for c, b in zip(COUNTERS, before)]
        assert np.array_equal(got[0], ref[0]), f"{ctx} route {route}: ids differ from the allow-list reference"
        assert np.array_equal(got[1], ref[1]), f"{ctx} route {route}: scores differ from the allow-list reference"
        if allow is None or len(allow) >= 4096:
            masked = route == 2 and scan_ok and m > 0
            assert delta == [1, int(m > 0 and not masked), int(masked)], f"{ctx} route {route}: counters {delta}"
        else:
            assert delta == [1, int(m > 0), 0], f"{ctx} route {route}: a short allow-list is resolved on the host and gathered: {delta}"
    eng.setTuning("predicate_route", 0)
    if minScore is None:
        assert len(ref[0]) == min(min(max(k, 1), 10_000), m - dropped), f"{ctx}: {len(ref[0])} results for {m} passing rows"
    if parity and m > 0 and minScore is None:                                                          # (b)
        rows = np.flatnonzero(mask)
        ei, es, _, _ = oracle.search(s.metric, s.corpus[rows], s.ids[rows], query, k)
        _, es_all, _, _ = oracle.search(s.metric, s.corpus[rows], s.ids[rows], query, min(k + 10, 10_000))
        assert_parity(ref[0], ref[1], ei, es, all_exp_scores=es_all, ctx=ctx)
    return mask


# ---- 1. both routes on every mask, time range and top_k ----------------------------------------------------------------------------

@pytest.mark.parametrize("deny,name", [(B_HALF, "random half"), (1, "deleted"), (2, "superseded"), (4, "surrogate"), (7, "default FrameFilter"),
                                       (B_NONE, "all pass"), (B_ALL, "none pass"), (B_BUT_ONE, "one row"), (B_BUT_TAIL, "final partial chunk")])
def test_deny_masks(s384, deny, name):
    mask = check(s384, 10, deny=deny, ctx=name)
    if name == "one row":
        assert mask.sum() == 1 and mask[s384.one_row]
    if name == "final partial chunk":
        assert mask.sum() == 3 and mask[-3:].all()
    if name == "none pass":
        assert mask.sum() == 0
    if name == "all pass":
        assert mask.all()


def test_time_ranges(s384):
    s = s384
    t = s.ts
    assert check(s, 10, timeRange=(int(t[13]), int(t[8006])), ctx="mid-chunk ends").sum() == 8006 - 13      # rows 13 .. 8005
    assert check(s, 10, timeRange=(int(t[15_001]), None), ctx="after alone").sum() == s.n - 15_001
    assert check(s, 10, timeRange=(None, int(t[700])), ctx="before alone").sum() == 700
    # ts == after passes, ts == before fails (TimeRange.contains)
    m = check(s, 10, timeRange=(int(t[100]), int(t[105])), ctx="exclusive upper end")
    assert list(np.flatnonzero(m)) == [100, 101, 102, 103, 104]
    m = check(s, 10, timeRange=(-9_000, -8_000), ctx="negative timestamps")
    assert m.sum() == 1000 and (t[m] < 0).all()
    assert check(s, 10, timeRange=(I64_MIN, I64_MAX), ctx="int64 ends").sum() == s.n - 1                 # only ts == INT64_MAX fails
    assert check(s, 10, timeRange=(I64_MAX, None), ctx="after = INT64_MAX").sum() == 1
    assert check(s, 10, timeRange=(None, I64_MIN), ctx="before = INT64_MIN").sum() == 0
    assert check(s, 10, timeRange=(int(t[13]), int(t[8006])), deny=7 | B_HALF, ctx="range and flags").sum() > 0


@pytest.mark.parametrize("k", [1, 10, 64, 65, 192, 193])
def test_top_k_values(s384, k):
    check(s384, k, deny=B_HALF, ctx=f"top_k {k}", q=1)                 # 193 takes the gather route on both settings (check's counters)


def test_top_k_larger_than_the_passing_rows(s384):
    m = check(s384, 10, timeRange=(int(s384.ts[40]), int(s384.ts[45])), ctx="5 rows pass", q=2)
    assert m.sum() == 5
    m = check(s384, 100, timeRange=(int(s384.ts[4_000]), int(s384.ts[4_070])), ctx="70 rows pass, top_k 100", q=2)
    assert m.sum() == 70


def test_768_and_generic_dims(s768, s100):
    for s in (s768, s100):
        check(s, 10, deny=B_HALF, ctx=f"{s.dims}-d random half")
        check(s, 65, timeRange=(int(s.ts[13]), int(s.ts[s.n // 2 + 5])), ctx=f"{s.dims}-d range", q=1)
        check(s, 10, deny=B_BUT_ONE, ctx=f"{s.dims}-d one row")
        check(s, 300, deny=7, ctx=f"{s.dims}-d top_k 300", q=2)


@pytest.mark.parametrize("metric", [1, 2])
def test_dot_and_l2(wax, metric):
    s = Store(wax, metric, 3_001, 384, seed=4 + metric)
    check(s, 10, deny=B_HALF, ctx=f"metric {metric} random half")
    check(s, 100, timeRange=(int(s.ts[13]), int(s.ts[2_005])), deny=7, ctx=f"metric {metric} range", q=1)
    s.eng.close()


# ---- 2. composition ----------------------------------------------------------------------------------------------------------------

def test_predicate_and_allow_list(s384):
    s = s384
    rng = np.random.default_rng(5)
    short = np.concatenate([s.ids[rng.choice(s.n, 300, replace=False)], np.array([1, 2, 10 ** 9], dtype=np.uint64)])
    long_ = np.concatenate([s.ids[rng.choice(s.n, 6_000, replace=False)], np.arange(10 ** 9, 10 ** 9 + 50, dtype=np.uint64)])
    long_ = np.concatenate([long_, long_[:40]])                        # repeats and absent ids
    assert len(short) < 4096 <= len(long_)
    for lst, name in ((short, "short list"), (long_, "long list")):
        assert check(s, 10, deny=B_HALF | 7, allow=lst, ctx=name).sum() > 0
        check(s, 70, timeRange=(int(s.ts[13]), int(s.ts[8_006])), allow=lst, ctx=name + " and range", q=1)
        assert check(s, 10, deny=B_ALL, allow=lst, ctx=name + ", none pass").sum() == 0
    assert len(s.eng.searchFiltered(s.queries[0], 10, frameIds=[], denyFlags=1)[0]) == 0     # an empty list allows nothing


def test_predicate_and_min_score(s384):
    s = s384
    ids, scores = s.eng.searchFiltered(s.queries[3], 50, denyFlags=B_HALF)
    assert len(ids) == 50
    cut = float(scores[20])
    for route in (1, 2):
        s.eng.setTuning("predicate_route", route)
        gi, gs = s.eng.searchFiltered(s.queries[3], 50, minScore=cut, denyFlags=B_HALF)
        keep = scores >= cut
        assert np.array_equal(gi, ids[keep]) and np.array_equal(gs, scores[keep]) and 21 <= len(gi) < 50
    s.eng.setTuning("predicate_route", 0)
    check(s, 50, deny=B_HALF, minScore=cut, q=3, ctx="min score")


def test_duplicates_nan_and_zero_rows(wax):
    n, dims = 2_003, 384
    s = Store(wax, 0, n, dims, seed=9)
    q = s.queries[0]
    dup_rows = [5, 777, 778, 1500, 2002]
    corpus = s.corpus.copy()
    for r in dup_rows:
        corpus[r] = q                                                  # five copies of the best possible row
    corpus[300] = 0.0                                                  # a zero row: cosine scores it 0
    corpus[301, 7] = np.nan                                            # a NaN row: its norm is NaN, so the scan's rule scores it 0 too
    s.corpus = corpus
    for r in dup_rows + [300, 301]:
        s.eng.add(int(s.ids[r]), corpus[r])                            # upserts keep the rows' attributes
    ts, fl, found = s.eng.getAttributes(s.ids)
    assert found.all() and np.array_equal(ts, s.ts) and np.array_equal(fl, s.fl)
    deny = int(s.fl[5]) & 7                                            # whatever low bits row 5 has: make the duplicates pass or fail together
    for r in dup_rows:
        s.fl[r] = s.fl[5]
    s.eng.setAttributes(s.ids[dup_rows], flags=s.fl[dup_rows])
    mask = check(s, 10, deny=(7 & ~deny) | B_NONE, ctx="duplicates", parity=False)
    assert mask[dup_rows].all()
    for route in (1, 2):
        s.eng.setTuning("predicate_route", route)
        gi, gs = s.eng.searchFiltered(q, 10, denyFlags=(7 & ~deny) | B_NONE)
        assert [int(i) for i in gi[:5]] == [int(s.ids[r]) for r in dup_rows], "equal vectors come back in ascending row order"
        assert len(set(gs[:5].tolist())) == 1
        # rows 250 .. 349 pass: the zero row and the NaN row score exactly as search scores them
        rng_ = (int(s.ts[250]), int(s.ts[350]))
        gi, gs = s.eng.searchFiltered(q, 200, timeRange=rng_)
        assert len(gi) == 100
        all_ids, all_scores = s.eng.searchArrays(q, 10_000)
        want = {int(i): float(v) for i, v in zip(all_ids, all_scores)}
        assert all(want[int(i)] == float(v) for i, v in zip(gi, gs)), "a passing row scores exactly as search scores it"
        for r in (300, 301):
            assert float(gs[list(gi).index(int(s.ids[r]))]) == want[int(s.ids[r])] == 0.0
    s.eng.setTuning("predicate_route", 0)
    check(s, 200, timeRange=(int(s.ts[250]), int(s.ts[350])), ctx="nan and zero rows", parity=False)
    s.eng.close()


# ---- 3. chunk skipping -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["s384", "s768"])
def test_chunk_skipping(request, which):
    s = request.getfixturevalue(which)
    lo = s.n // 3 + 3                                                  # mid-chunk on purpose
    hi = lo + s.n // 16
    s.eng.setTuning("predicate_route", 2)
    b0, k0, m0 = s.eng.stats().bytes_scanned, s.eng.getTuning("predicate_chunks_skipped"), s.eng.getTuning("predicate_masked_scans")
    gi, _ = s.eng.searchFiltered(s.queries[0], 10, timeRange=(int(s.ts[lo]), int(s.ts[hi])))
    s.eng.setTuning("predicate_route", 0)
    assert len(gi) == 10 and s.eng.getTuning("predicate_masked_scans") == m0 + 1
    passing = hi - lo
    assert s.eng.stats().bytes_scanned - b0 <= (passing + 16) * s.dims * 4
    c = CHUNK[s.dims]
    n_chunks = -(-s.n // c)
    live = len(set(range(lo // c, (hi - 1) // c + 1)))
    assert s.eng.getTuning("predicate_chunks_skipped") - k0 == n_chunks - live


# ---- 4. attributes follow the store ------------------------------------------------------------------------------------------------

def test_attributes_follow_the_store(wax):
    dims = 128
    rng = np.random.default_rng(11)
    pool = corpus_for(0, 400, dims, seed=12)
    eng = wax.HIPVectorEngine(metric=wax.VectorMetric(0), dimensions=dims)
    q = oracle.gaussian_unit_queries(2, dims)[0]
    model = {}                                                        # frame id -> [vector row of `pool`, ts, flags], insertion order = row order
    order = []

    def verify(ctx):
        ids = np.array(order, dtype=np.uint64)
        ts, fl, found = eng.getAttributes(np.concatenate([ids, np.array([10 ** 12], dtype=np.uint64)]))
        assert found[:-1].all() and not found[-1] and ts[-1] == 0 and fl[-1] == 0, ctx
        mts = np.array([model[i][1] for i in order], dtype=np.int64)
        mfl = np.array([model[i][2] for i in order], dtype=np.uint32)
        assert np.array_equal(ts[:-1], mts) and np.array_equal(fl[:-1], mfl), f"{ctx}: getAttributes"
        for tr, deny in (((10, 60), 0), (None, 1), ((None, 1), 2), ((0, None), 5)):
            m = (mfl & np.uint32(deny)) == 0
            if tr is not None:
                m &= (mts >= tr[0]) if tr[0] is not None else True
                m &= (mts < tr[1]) if tr[1] is not None else True
            ref = eng.searchFiltered(q, 20, frameIds=ids[m])
            for route in (1, 2):
                eng.setTuning("predicate_route", route)
                got = eng.searchFiltered(q, 20, timeRange=tr, denyFlags=deny)
                assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), f"{ctx}: {tr} deny {deny} route {route}"
            eng.setTuning("predicate_route", 0)
            assert len(ref[0]) == min(20, int(m.sum())), ctx

    def add(first, count, batch=True):
        ids = np.arange(first, first + count, dtype=np.uint64)
        if batch:
            eng.addBatch(ids, pool[first:first + count])
        else:
            for i in ids:
                eng.add(int(i), pool[int(i)])
        for i in ids:
            model[int(i)] = [int(i), 0, 0]
            order.append(int(i))

    def set_attrs(ids, ts=None, fl=None):
        assert eng.setAttributes(np.array(ids, dtype=np.uint64), ts, fl) == len(ids)
        for j, i in enumerate(ids):
            if ts is not None:
                model[i][1] = int(ts[j])
            if fl is not None:
                model[i][2] = int(fl[j])

    add(0, 50)                                                         # capacity 64
    assert eng.getTuning("attr_device_rows") == 0
    set_attrs(list(range(50)), ts=np.arange(50), fl=rng.integers(0, 8, 50))
    verify("after setAttributes")
    assert eng.getTuning("attr_device_rows") >= 50
    up0 = eng.getTuning("attr_uploaded_rows")
    add(50, 7, batch=False)                                            # appended rows are (0, 0); still capacity 64
    verify("after add")
    assert eng.getTuning("attr_uploaded_rows") - up0 == 7, "an append uploads only its own rows"
    eng.add(3, pool[399])                                              # upsert: same frame, same attributes
    verify("after an upsert")
    assert eng.getTuning("attr_uploaded_rows") - up0 == 7
    eng.remove(10); order.remove(10); del model[10]
    verify("after remove")
    gone = [0, 4, 5, 30, 56, 12345]
    assert eng.removeBatch(gone) == 5
    for i in gone[:-1]:
        order.remove(i); del model[i]
    verify("after removeBatch")
    add(57, 200)                                                       # 51 -> 251 rows: capacity 64 -> 128 -> 256
    assert eng.stats().reserved_rows == 256
    verify("after growth across two capacity doublings")
    set_attrs([60, 61, 200], ts=[55, 56, 57], fl=[1, 2, 4])
    verify("after setAttributes on appended rows")
    eng.reserve(1000)
    assert eng.stats().reserved_rows >= 1000
    verify("after reserve")
    set_attrs([1, 2, 3, 60], fl=[7, 0, 1 << 20, 0])                    # flags only: timestamps stay
    verify("after a flags-only setAttributes")
    set_attrs([1, 1], ts=[5, 40])                                      # an id listed twice: the last entry wins
    assert model[1][1] == 40
    verify("after a repeated id")
    assert eng.setAttributes([10 ** 12, 2], [1, 41]) == 1              # unknown ids are skipped
    model[2][1] = 41
    verify("after an unknown id")
    blob = eng.serialize()
    eng.deserialize(blob)
    for i in order:
        model[i][1], model[i][2] = 0, 0
    verify("after deserialize")
    eng.close()


# ---- 5. a store that never had attributes ------------------------------------------------------------------------------------------

def test_store_without_attributes(wax):
    n, dims = 3_001, 384
    corpus = corpus_for(0, n, dims, seed=21)
    eng = wax.HIPVectorEngine(metric=wax.VectorMetric(0), dimensions=dims)
    eng.addBatch(np.arange(n, dtype=np.uint64), corpus)
    q = oracle.gaussian_unit_queries(1, dims)[0]
    plain = eng.searchArrays(q, 10)
    for route in (1, 2):
        eng.setTuning("predicate_route", route)
        got = eng.searchFiltered(q, 10, denyFlags=7)                   # every row is (0, 0): nothing is denied
        assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1])
        assert len(eng.searchFiltered(q, 10, timeRange=(1, None))[0]) == 0      # after = 1 passes nothing
        got = eng.searchFiltered(q, 10, timeRange=(0, 1))
        assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1])
    assert eng.getTuning("predicate_searches") == 6
    assert eng.getTuning("attr_device_rows") == 0 and eng.getTuning("attr_uploaded_rows") == 0, "no attribute memory is allocated"
    ts, fl, found = eng.getAttributes([0, 5, n])
    assert list(ts) == [0, 0, 0] and list(fl) == [0, 0, 0] and list(found) == [True, True, False]
    eng.close()


# ---- 6. nothing else moves ---------------------------------------------------------------------------------------------------------

def test_nothing_else_moves(wax):
    n, dims = 3_001, 384
    corpus = corpus_for(0, n, dims, seed=22)
    ids = np.arange(n, dtype=np.uint64) + 100
    eng = wax.HIPVectorEngine(metric=wax.VectorMetric(0), dimensions=dims)
    eng.addBatch(ids, corpus)
    qs = oracle.gaussian_unit_queries(20, dims)
    allow = ids[::3]

    def snapshot():
        return (eng.searchArrays(qs[0], 10), eng.searchArrays(qs[1], 300), eng.searchBatch(qs, 10), eng.searchFiltered(qs[2], 10, frameIds=allow),
                eng.searchFiltered(qs[3], 10, minScore=0.05), eng.searchFiltered(qs[4], 10, timeRange=None, denyFlags=0), eng.serialize())

    before = snapshot()
    n0 = eng.getTuning("predicate_searches")
    rng = np.random.default_rng(23)
    eng.setAttributes(ids, rng.integers(-5, 5, n), rng.integers(0, 1 << 12, n))
    after = snapshot()
    assert eng.getTuning("predicate_searches") == n0, "a call without the new arguments goes through the old entry"
    for b, a in zip(before[:-1], after[:-1]):
        for x, y in zip(b, a):
            assert np.array_equal(x, y)
    assert before[-1] == after[-1], "serialize() bytes are unchanged by setAttributes"
    eng.close()


# ---- 7. three shards on one GPU ----------------------------------------------------------------------------------------------------

def test_three_shards_equal_the_single_engine(wax):
    one = Store(wax, 0, 3_072, 384, seed=31)
    many = Store(wax, 0, 3_072, 384, seed=31, devices=[0, 0, 0])
    assert [many.eng.shardInfo(g)[2] for g in range(3)] == [1024, 1024, 1024]
    ts, fl, found = many.eng.getAttributes(many.ids[::-1])
    assert found.all() and np.array_equal(ts, many.ts[::-1]) and np.array_equal(fl, many.fl[::-1])
    for route in (0, 1, 2):
        for e in (one.eng, many.eng):
            e.setTuning("predicate_route", route)
        for k in (10, 100):
            for tr, deny in ((None, B_HALF), ((int(one.ts[13]), int(one.ts[2_006])), 0), ((int(one.ts[1_000]), int(one.ts[1_030])), 7)):
                a = one.eng.searchFiltered(one.queries[0], k, timeRange=tr, denyFlags=deny)
                b = many.eng.searchFiltered(one.queries[0], k, timeRange=tr, denyFlags=deny)
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), f"route {route} k {k} {tr} {deny}"
                assert len(a[0]) == min(k, int(one.passing(tr, deny).sum()))
    assert many.eng.getTuning("predicate_searches") == 3 * 18        # every shard answers every query; counters are summed
    assert many.eng.getTuning("predicate_masked_scans") > 0 and many.eng.getTuning("predicate_gather_searches") > 0
    # a removal in the middle shard: its attributes move with its rows
    gone = many.ids[1024:1500]
    for s in (one, many):
        assert s.eng.removeBatch(gone) == len(gone)
    a = one.eng.searchFiltered(one.queries[1], 50, denyFlags=B_HALF | 7)
    b = many.eng.searchFiltered(one.queries[1], 50, denyFlags=B_HALF | 7)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and not set(gone.tolist()) & set(b[0].tolist())
    one.eng.close()
    many.eng.close()


def test_rebalance_carries_the_attributes(wax):
    """A handle that grows by doubling moves whole shards (sh_move_all): the attribute columns travel with the rows."""
    dims = 128
    one = wax.HIPVectorEngine(metric=wax.VectorMetric(0), dimensions=dims)
    many = wax.HIPVectorEngine(metric=wax.VectorMetric(0), dimensions=dims, devices=[0, 0, 0])
    many.setTuning("shard_min_mb", 0)
    corpus = corpus_for(0, 9_000, dims, seed=41)
    q = oracle.gaussian_unit_queries(2, dims)
    ts_of = lambda ids: ids.astype(np.int64) * 7 - 20_000                 # noqa: E731
    fl_of = lambda ids: ((ids * 2654435761) >> 7).astype(np.uint32) & np.uint32(0x30f)   # noqa: E731
    done = 0
    for step in (100, 700, 64, 3000, 1, 5135):
        ids = np.arange(done, done + step, dtype=np.uint64)
        for eng in (one, many):
            eng.addBatch(ids, corpus[done:done + step])
            if step != 64:                                             # one batch keeps its (0, 0): it must stay so through the moves
                assert eng.setAttributes(ids, ts_of(ids), fl_of(ids)) == step
        done += step
        for route in (1, 2):
            for eng in (one, many):
                eng.setTuning("predicate_route", route)
            for tr, deny in ((None, 0x100), ((-15_000, 9_000), 0), ((0, 1), 7), (None, 0x20f)):
                a = one.searchFiltered(q[0], 40, timeRange=tr, denyFlags=deny)
                b = many.searchFiltered(q[0], 40, timeRange=tr, denyFlags=deny)
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), f"{done} rows, route {route}, {tr}, {deny}"
    assert many.getTuning("rebalances") >= 1 and many.getTuning("shards") == 3
    ids = np.arange(done, dtype=np.uint64)
    ts, fl, found = many.getAttributes(ids)
    want_ts, want_fl = ts_of(ids), fl_of(ids)
    want_ts[800:864], want_fl[800:864] = 0, 0
    assert found.all() and np.array_equal(ts, want_ts) and np.array_equal(fl, want_fl)
    one.close()
    many.close()


def test_auto_rule_decides_by_the_passing_fraction(s384):
    """"predicate_route" 0: the masked scan where it is eligible and at least "predicate_scan_min_permille" rows per thousand pass."""
    s, eng = s384, s384.eng
    default = eng.getTuning("predicate_scan_min_permille")
    assert 0 <= default <= 1001 and eng.getTuning("predicate_route") == 0

    def route_of(k=10, **kw):
        before = [eng.getTuning(c) for c in COUNTERS]
        eng.searchFiltered(s.queries[0], k, **kw)
        d = [eng.getTuning(c) - b for c, b in zip(COUNTERS, before)]
        assert d[0] == 1 and d[1] + d[2] == 1, d
        return "masked" if d[2] else "gather"

    half = int(s.passing(deny=B_HALF).sum()) * 1000 // s.n            # about 500 rows per thousand
    narrow = (int(s.ts[5_000]), int(s.ts[5_000 + s.n // 16]))          # 62 per thousand
    try:
        eng.setTuning("predicate_scan_min_permille", half - 50)
        assert route_of(denyFlags=B_HALF) == "masked" and route_of(timeRange=narrow) == "gather"
        assert route_of(k=193, denyFlags=B_HALF) == "gather"          # never eligible above 192
        eng.setTuning("predicate_scan_min_permille", half + 50)
        assert route_of(denyFlags=B_HALF) == "gather" and route_of(denyFlags=B_NONE) == "masked"
        eng.setTuning("predicate_scan_min_permille", 62)              # exactly n // 16 of n rows: 62.47 per thousand passes 62, not 63
        assert route_of(timeRange=narrow) == "masked"
        eng.setTuning("predicate_scan_min_permille", 63)
        assert route_of(timeRange=narrow) == "gather"
        eng.setTuning("predicate_scan_min_permille", 0)
        assert route_of(denyFlags=B_BUT_ONE) == "masked"
        eng.setTuning("predicate_scan_min_permille", 1001)
        assert route_of(denyFlags=B_NONE) == "gather"
        eng.setTuning("force_general", 1)
        eng.setTuning("predicate_scan_min_permille", 0)
        assert route_of(denyFlags=B_HALF) == "gather"
    finally:
        eng.setTuning("force_general", 0)
        eng.setTuning("predicate_scan_min_permille", default)


# ---- 8. errors ---------------------------------------------------------------------------------------------------------------------

def test_errors(wax, hip_lib, s384):
    s = s384
    eng = s.eng
    ticket = eng.submit(s.queries[0], 10)
    try:
        with pytest.raises(wax.EncodingError, match="collect outstanding search tickets first"):
            eng.setAttributes(s.ids[:3], [1, 2, 3])                    # refused, not deadlocked: this thread holds the read lock
    finally:
        eng.collect(ticket, 10)
    assert eng.setAttributes(s.ids[:3], s.ts[:3]) == 3
    with pytest.raises(wax.EncodingError, match="vector dimension mismatch: expected 384, got 100"):
        eng.searchFiltered(np.zeros(100, dtype=np.float32), 10, denyFlags=1)
    with pytest.raises(wax.EncodingError, match="one timestamp / flag word per frame id"):
        eng.setAttributes(s.ids[:3], [1, 2])
    f32, u64 = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint64)
    from wax_amd import _abi
    pred = _abi.RowPredicate(0, 0, 0, 0, 1)
    got = ctypes.c_uint32(9)
    q = s.queries[0]
    out_i, out_s = np.zeros(10, dtype=np.uint64), np.zeros(10, dtype=np.float32)
    rc = hip_lib.wax_hip_search_predicate(eng._h, None, 384, 10, 0, None, 0, 0, 0.0, ctypes.byref(pred), out_i.ctypes.data_as(u64),
                                          out_s.ctypes.data_as(f32), 10, ctypes.byref(got))
    assert rc == -7 and got.value == 0
    rc = hip_lib.wax_hip_search_predicate(eng._h, q.ctypes.data_as(f32), 384, 10, 0, None, 0, 0, 0.0, ctypes.byref(pred), None, None, 10,
                                          ctypes.byref(got))
    assert rc == -7
    rc = hip_lib.wax_hip_search_predicate(eng._h, q.ctypes.data_as(f32), 384, 10, 1, None, 5, 0, 0.0, ctypes.byref(pred),
                                          out_i.ctypes.data_as(u64), out_s.ctypes.data_as(f32), 10, ctypes.byref(got))
    assert rc == -7 and b"allow-list is null" in hip_lib.wax_hip_last_error()
    assert hip_lib.wax_hip_set_attributes(eng._h, None, None, None, 3, None) == -7
    assert hip_lib.wax_hip_get_attributes(eng._h, None, 3, None, None, None) == -7
    # a null predicate is the filtered search
    rc = hip_lib.wax_hip_search_predicate(eng._h, q.ctypes.data_as(f32), 384, 10, 0, None, 0, 0, 0.0, None, out_i.ctypes.data_as(u64),
                                          out_s.ctypes.data_as(f32), 10, ctypes.byref(got))
    plain = eng.searchArrays(q, 10)
    assert rc == 0 and got.value == 10 and np.array_equal(out_i, plain[0]) and np.array_equal(out_s, plain[1])
    with pytest.raises(wax.EncodingError, match="predicate_route"):
        eng.setTuning("predicate_route", 3)
