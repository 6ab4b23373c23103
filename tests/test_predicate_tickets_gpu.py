"""Predicate tickets (wax_hip_search_predicate_submit / HIPVectorEngine.submitFiltered): a predicate search as a ticket of
the ordinary collect, riding masked passes over the 8-bit code mirror (mirror8_scan_masked_group_kernel) in the sets the unfiltered
mirror tickets form, or deferred to the blocking body.

Every collected answer is compared array_equal (ids and scores) with the blocking searchFiltered on the same engine. The counters of
predicateTicketStats() and the existing mirror counters say which way a ticket went. Stores, queries and most masks are
predicate_mirror_ref's (20 005 x 384 and 3 001 x 768, cosine and dot: neither row count is a multiple of 16 or 32); the engines run
under "predicate_mirror" 2, "mirror_bits" 8, "scan_mirror" 2 and "mirror_share" 2, so a set is exactly what a test parks: tickets wait
until four are parked or one of them is collected.

Zero fallbacks are asserted only where the float64 model of the 8-bit certificate (mirror8_ref: quantise, lower_bounds, slack; MaskedModel:
the 64 best passing lower bounds and their exact k-th distance) leaves lb_64 - slack - d_k >= MARGIN_FLOOR — the f32-against-f64 error
that floor was sized for is <= 5.5e-4 — and that margin is asserted first, so a failure names the side that moved."""
import functools
import threading

import numpy as np
import pytest

import mirror8_ref as M8
import predicate_mirror_ref as R

pytestmark = pytest.mark.gpu

KS = (1, 10, 16)
SET_SIZES = (1, 2, 3, 4, 1, 2, 3)               # 16 queries: every set size, the small ones twice
BIT_ROT16, BIT_EVEN, BIT_ODD = 1 << 16, 1 << 17, 1 << 18
TILE = 16                                       # rows per tile of the 8-bit pass
STAT_KEYS = ("submitted", "rode", "masked_passes", "certified", "fallbacks", "deferred", "host_decided", "bitmap_builds", "bitmap_hits")


# ---- masks of this file ----------------------------------------------------------------------------------------------------------------

def rot16_mask(n):
    """Exactly one passing row per 16-row tile, at position tile % 16 (a ragged last tile that does not reach its position has none):
    over 16 tiles every lane position is the only offer once, and odd tiles sit in the upper half of their bitmap word."""
    rows = np.arange(0, n, TILE) + (np.arange(0, n, TILE) // TILE) % TILE
    m = np.zeros(n, dtype=bool)
    m[rows[rows < n]] = True
    return m


def tile_parity_mask(n, parity):
    return ((np.arange(n) // TILE) % 2) == parity


def flags_of(n, dims):
    fl = R.flags_for(n, dims).copy()
    fl[~rot16_mask(n)] |= np.uint32(BIT_ROT16)
    fl[~tile_parity_mask(n, 0)] |= np.uint32(BIT_EVEN)
    fl[~tile_parity_mask(n, 1)] |= np.uint32(BIT_ODD)
    return fl


def predicate_of(n, name):
    """mask name -> the keyword arguments of searchFiltered / submitFiltered."""
    if name == "range":
        return {"timeRange": R.range_bounds(n)}
    if name == "rot16":
        return {"denyFlags": BIT_ROT16}
    if name == "lower":
        return {"timeRange": (None, n // 2)}
    if name == "upper":
        return {"timeRange": (n // 2, None)}
    if name == "even_tiles":
        return {"denyFlags": BIT_EVEN}
    if name == "odd_tiles":
        return {"denyFlags": BIT_ODD}
    return {"denyFlags": R.MASK_BIT[name]}


def mask_of(n, dims, name):
    if name == "rot16":
        return rot16_mask(n)
    if name == "all":
        return np.ones(n, dtype=bool)
    return R.masks(n, dims)[name]


# ---- the float64 model of the masked 8-bit certificate ---------------------------------------------------------------------------------

Model8 = M8.MaskedModel          # (shared with masked_iterations_ref.py)


@functools.lru_cache(maxsize=None)
def model8(name):
    metric, _, dims = R.STORES[name]
    return Model8(metric, R.store_rows(name), R.queries(dims))


# ---- engines ----------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def wax(hip_lib):
    import wax_amd
    if hip_lib.wax_hip_device_count() == 0:
        pytest.skip("no HIP device on this host: the gpu-marked tests run on the MI355X box (pytest -m gpu)")
    assert hip_lib.wax_hip_available() == 1, "a HIP device is visible but it is not gfx950: the HIP path needs an MI355X"
    return wax_amd


def warm_code_mirror(eng, q):
    """A stale or missing code mirror is rebuilt by the third query in a row that wants it (mirror8_take): three unfiltered searches."""
    for _ in range(3):
        eng.searchArrays(q, 1)


class Store:
    """An engine over rows with ts = row and a flag column (a row fails a mask iff the mask's bit is set), set up so that the test
    decides the sets."""

    def __init__(self, wax, metric, rows, flags=None, attributes=True, predicate_mirror=2, **kw):
        self.metric, (self.n, self.dims) = metric, rows.shape
        self.rows = np.array(rows)
        self.ids = np.arange(self.n, dtype=np.uint64) * 3 + 7
        self.ts = np.arange(self.n, dtype=np.int64)
        self.fl = np.zeros(self.n, dtype=np.uint32) if flags is None else np.array(flags, dtype=np.uint32)
        self.eng = wax.HIPVectorEngine(metric=wax.VectorMetric(metric), dimensions=self.dims, **kw)
        if kw.get("devices"):
            self.eng.setTuning("shard_min_mb", 0)
        self.eng.addBatch(self.ids, self.rows)
        if attributes:
            assert self.eng.setAttributes(self.ids, self.ts, self.fl) == self.n
        for key, value in (("predicate_mirror", predicate_mirror), ("mirror_bits", 8), ("scan_mirror", 2), ("mirror_share", 2)):
            self.eng.setTuning(key, value)
        self.queries = R.queries(self.dims) if self.dims in (384, 768) else None

    def stats(self):
        return self.eng.predicateTicketStats()

    def delta(self, before):
        now = self.stats()
        return {k: now[k] - before[k] for k in STAT_KEYS}

    def passing(self, timeRange=None, denyFlags=0):
        m = (self.fl & np.uint32(denyFlags)) == 0
        if timeRange is not None:
            if timeRange[0] is not None:
                m &= self.ts >= timeRange[0]
            if timeRange[1] is not None:
                m &= self.ts < timeRange[1]
        return m


@pytest.fixture(scope="module")
def stores(wax):
    made = {}

    def get(name):
        if name not in made:
            metric, n, dims = R.STORES[name]
            s = Store(wax, metric, R.store_rows(name), flags_of(n, dims))
            warm_code_mirror(s.eng, s.queries[0])
            made[name] = s
        return made[name]

    yield get
    for s in made.values():
        s.eng.close()


def blocking(s, q, k, **pred):
    """The reference of every ticket: the blocking call on the same engine (an empty predicate: the unfiltered search)."""
    query = s.queries[q] if np.ndim(q) == 0 else q
    if not pred:
        return s.eng.searchArrays(query, k)
    return s.eng.searchFiltered(query, k, **pred)


def assert_same(got, ref, ctx):
    assert np.array_equal(got[0], ref[0]), f"{ctx}: ids {got[0]} != {ref[0]}"
    assert np.array_equal(got[1], ref[1]), f"{ctx}: scores differ"


def run_set(s, members, k):
    """Park the members — (query index, predicate kwargs; {} = an unfiltered ticket) — and collect them in order: one set of
    mirror_share 2 (at most four). Returns the answers."""
    assert 1 <= len(members) <= 4
    tickets = [s.eng.submitFiltered(s.queries[q], k, **pred) if pred else s.eng.submit(s.queries[q], k) for q, pred in members]
    return [s.eng.collect(t, k) for t in tickets]


# ---- 1. taken masks: every mask, k and set size rides, is certified and equals the blocking call -------------------------------------------

@pytest.mark.parametrize("name", list(R.STORES))
def test_taken_masks_ride_certified_in_sets_of_one_to_four(stores, name):
    s = stores(name)
    model = model8(name)
    for mask_name in R.TAKEN_MASKS + ("rot16",):
        pred = predicate_of(s.n, mask_name)
        mask = mask_of(s.n, s.dims, mask_name)
        assert np.array_equal(s.passing(**pred), mask), mask_name
        if mask_name == "rot16":
            tiles = np.add.reduceat(mask.astype(np.int64), np.arange(0, s.n, TILE))
            assert tiles[:-1].tolist() == [1] * (len(tiles) - 1) and mask[np.arange(16) * TILE + np.arange(16)].all()
        for k in KS:
            margins = [model.margin(mask, q, k) for q in range(R.N_QUERIES)]
            print(f"{name} {mask_name} top_k {k}: smallest model margin {min(margins):.4f}")
            assert min(margins) >= R.MARGIN_FLOOR, f"{name} {mask_name} top_k {k}: the model does not certify (margin {min(margins)})"
            refs = [blocking(s, q, k, **pred) for q in range(R.N_QUERIES)]
            before, p8 = s.stats(), s.eng.getTuning("mirror8_passes")
            got, q0 = [], 0
            for size in SET_SIZES:
                got += run_set(s, [(q, pred) for q in range(q0, q0 + size)], k)
                q0 += size
            assert q0 == R.N_QUERIES
            d = s.delta(before)
            ctx = f"{name} {mask_name} top_k {k}"
            for q in range(R.N_QUERIES):
                assert_same(got[q], refs[q], f"{ctx} query {q}")
                assert len(got[q][0]) == min(k, int(mask.sum())), ctx
            assert d["submitted"] == R.N_QUERIES and d["rode"] == d["submitted"] and d["fallbacks"] == 0 and d["deferred"] == 0, f"{ctx}: {d}"
            assert d["certified"] == R.N_QUERIES, f"{ctx}: {d}"
            assert d["masked_passes"] == len(SET_SIZES), f"{ctx}: {d}"
            assert s.eng.getTuning("mirror8_passes") - p8 == len(SET_SIZES), ctx
    assert s.eng.getTuning("mirror8_breaker_trips") == 0


# ---- 2. a mixed set: an unfiltered member beside three masks, one pass -------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cos384", "dot768"])
def test_a_mixed_set_is_one_pass_and_every_member_its_own_answer(stores, name):
    s = stores(name)
    model = model8(name)
    members = [(0, {}), (1, predicate_of(s.n, "half")), (2, predicate_of(s.n, "r15")), (3, predicate_of(s.n, "range"))]
    for k in KS:
        for (q, pred), mask_name in zip(members, ("all", "half", "r15", "range")):
            assert model.margin(mask_of(s.n, s.dims, mask_name), q, k) >= R.MARGIN_FLOOR, (mask_name, k)
        refs = [blocking(s, q, k, **pred) for q, pred in members]
        before = s.stats()
        counters = [s.eng.getTuning(c) for c in ("mirror_passes", "mirror8_passes", "mirror_shared_passes", "mirror_shared_queries", "mirror8_fallbacks")]
        got = run_set(s, members, k)
        d = s.delta(before)
        moved = [s.eng.getTuning(c) - v for c, v in zip(("mirror_passes", "mirror8_passes", "mirror_shared_passes", "mirror_shared_queries", "mirror8_fallbacks"), counters)]
        for i in range(4):
            assert_same(got[i], refs[i], f"{name} top_k {k} member {i}")
        assert moved == [1, 1, 1, 4, 0], moved
        assert d["submitted"] == 3 and d["rode"] == 3 and d["masked_passes"] == 1 and d["certified"] == 3 and d["fallbacks"] == 0, d


# ---- 3. disjoint members ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cos384", "dot768"])
def test_disjoint_members_see_only_their_own_rows(stores, name):
    s = stores(name)
    sets = [[(0, predicate_of(s.n, "even_tiles")), (1, predicate_of(s.n, "odd_tiles"))],
            [(2, predicate_of(s.n, "lower")), (3, predicate_of(s.n, "upper"))],
            [(4, predicate_of(s.n, "tail_plus_65")), (5, {})],
            [(6, predicate_of(s.n, "odd_tiles")), (6, predicate_of(s.n, "even_tiles")), (6, predicate_of(s.n, "upper")), (6, predicate_of(s.n, "tail_plus_65"))]]
    assert not (tile_parity_mask(s.n, 0) & tile_parity_mask(s.n, 1)).any()
    for members in sets:
        for k in (1, 16):
            refs = [blocking(s, q, k, **pred) for q, pred in members]
            before = s.stats()
            got = run_set(s, members, k)
            d = s.delta(before)
            for (q, pred), g, r in zip(members, got, refs):
                assert_same(g, r, f"{name} {pred} top_k {k}")
                if pred:
                    allowed = set(s.ids[s.passing(**pred)].tolist())
                    assert set(g[0].tolist()) <= allowed, f"{name} {pred}: a denied row in the answer"
            assert d["masked_passes"] == 1 and d["rode"] == d["submitted"] == sum(1 for _, p in members if p), d


# ---- 4. masks of 64 rows and of none: never certified, and silent towards the breaker -----------------------------------------------------------

def test_masks_of_64_rows_or_none_are_answered_by_the_blocking_body_and_do_not_feed_the_breaker(stores):
    s = stores("cos384")
    assert int(s.passing(**predicate_of(s.n, "m64")).sum()) == 64 and int(s.passing(**predicate_of(s.n, "m0")).sum()) == 0
    before, trips = s.stats(), s.eng.getTuning("mirror8_breaker_trips")
    for mask_name in ("m64", "m0"):
        pred = predicate_of(s.n, mask_name)
        refs = [blocking(s, q, 10, **pred) for q in range(4)]
        for round_ in range(5):
            got = run_set(s, [(q, pred) for q in range(4)], 10)
            for q in range(4):
                assert_same(got[q], refs[q], f"{mask_name} round {round_} query {q}")
    d = s.delta(before)
    assert d["submitted"] == 40 and d["certified"] == 0 and d["rode"] + d["deferred"] == 40 and d["fallbacks"] == d["rode"], d
    # 8 uncertified of 32 would trip it
    assert s.eng.getTuning("mirror8_breaker_trips") == trips == 0
    got = run_set(s, [(0, predicate_of(s.n, "half"))], 10)          # and the 8-bit route is still open
    assert_same(got[0], blocking(s, 0, 10, **predicate_of(s.n, "half")), "after the small masks")
    assert s.delta(before)["certified"] == 1


# ---- 5. tickets that do not ride ----------------------------------------------------------------------------------------------------------

def check_deferred(s, k, pred, ctx, queries=(0, 1, 2)):
    refs = [blocking(s, q, k, **pred) for q in queries]
    before = s.stats()
    tickets = [s.eng.submitFiltered(s.queries[q], k, **pred) for q in queries]
    got = [s.eng.collect(t, k) for t in tickets]
    d = s.delta(before)
    for g, r, q in zip(got, refs, queries):
        assert_same(g, r, f"{ctx} query {q}")
    assert d["submitted"] == len(queries) and d["deferred"] == len(queries) and d["rode"] == 0 and d["masked_passes"] == 0, f"{ctx}: {d}"


def test_top_k_above_16_is_deferred(stores):
    s = stores("cos384")
    for k in (17, 32, 300):
        check_deferred(s, k, predicate_of(s.n, "half"), f"top_k {k}")


def test_l2_other_dimensions_the_key_and_a_handle_are_deferred(wax, stores):
    rows, fl = R.store_rows("cos384")[:3_001], flags_of(20_005, 384)[:3_001]
    s = Store(wax, 2, rows, fl)
    check_deferred(s, 10, {"denyFlags": R.MASK_BIT["half"]}, "L2")
    s.eng.close()
    s = Store(wax, 0, np.ascontiguousarray(rows[:, :128]), fl)
    s.queries = np.ascontiguousarray(R.queries(384)[:, :128])
    check_deferred(s, 10, {"denyFlags": R.MASK_BIT["half"]}, "128-d")
    s.eng.close()
    s = stores("cos768")
    s.eng.setTuning("predicate_mirror", 0)
    try:
        check_deferred(s, 10, predicate_of(s.n, "r15"), "predicate_mirror 0")
    finally:
        s.eng.setTuning("predicate_mirror", 2)
    many = Store(wax, 0, s.rows, s.fl, devices=[0, 0])
    assert many.eng.getTuning("shards") == 2
    refs = [many.eng.searchFiltered(many.queries[q], 10, minScore=0.05, **predicate_of(s.n, "r15")) for q in range(3)]
    tickets = [many.eng.submitFiltered(many.queries[q], 10, minScore=0.05, **predicate_of(s.n, "r15")) for q in range(3)]
    got = [many.eng.collect(t, 10) for t in tickets]
    for q in range(3):
        assert_same(got[q], refs[q], f"two shards query {q}")
        assert_same(got[q], s.eng.searchFiltered(s.queries[q], 10, minScore=0.05, **predicate_of(s.n, "r15")), f"two shards against one engine, query {q}")
    st = many.stats()
    assert st["submitted"] == 3 and st["deferred"] == 3 and st["rode"] == 0
    t = many.eng.submitFiltered(many.queries[0], 5)                 # an empty predicate on a handle: the ordinary ticket
    assert_same(many.eng.collect(t, 5), many.eng.searchArrays(many.queries[0], 5), "handle, empty predicate")
    assert many.stats()["submitted"] == 3
    many.eng.close()


# ---- 6. bitmap entries --------------------------------------------------------------------------------------------------------------------

def test_bitmap_entries_follow_the_store(wax):
    dims, bit = 384, 1 << 8
    pool = R.store_rows("cos384")
    rng = np.random.default_rng(5)
    fl_pool = np.where(rng.random(len(pool)) < 0.25, bit, 0).astype(np.uint32)
    s = Store(wax, 0, pool[:3_001], fl_pool[:3_001])
    eng, q, k = s.eng, s.queries[6], 10
    warm_code_mirror(eng, q)

    def ticket():
        return eng.collect(eng.submitFiltered(q, k, denyFlags=bit), k)

    before = s.stats()
    tickets = [eng.submitFiltered(s.queries[i], k, denyFlags=bit) for i in range(8)]
    got = [eng.collect(t, k) for t in tickets]
    for i in range(8):
        assert_same(got[i], eng.searchFiltered(s.queries[i], k, denyFlags=bit), f"eight tickets, query {i}")
    d = s.delta(before)
    assert d["bitmap_builds"] == 1 and d["bitmap_hits"] == 7 and d["rode"] == 8 and d["masked_passes"] == 2, d

    def mutated(what, mutate, gone=None):
        """After `mutate` the next ticket sees the store as it is now: one more build, the blocking answer."""
        builds = s.stats()["bitmap_builds"]
        mutate()
        warm_code_mirror(eng, q)          # (an upsert or a removal leaves the code mirror to its own rebuild rule)
        before = s.stats()
        got = ticket()
        d = s.delta(before)
        assert_same(got, eng.searchFiltered(q, k, denyFlags=bit), what)
        assert d["rode"] == 1 and d["bitmap_builds"] == 1 and s.stats()["bitmap_builds"] == builds + 1, f"{what}: {d}"
        if gone is not None:
            assert gone not in got[0].tolist(), what
        return got

    top = int(ticket()[0][0])
    mutated("setAttributes", lambda: eng.setAttributes([top], flags=[bit]), gone=top)
    new_ids = np.arange(10 ** 6, 10 ** 6 + 200, dtype=np.uint64)
    new_rows = pool[4_000:4_200].copy()
    new_rows[17] = q
    got = mutated("append", lambda: eng.addBatch(new_ids, new_rows))
    assert int(got[0][0]) == 10 ** 6 + 17                             # an appended row has attributes (0, 0): it passes
    got = mutated("upsert", lambda: eng.add(int(new_ids[17]), pool[5_000]), gone=10 ** 6 + 17)
    top = int(got[0][0])
    got = mutated("remove", lambda: eng.remove(top), gone=top)
    gone = got[0][:5]
    got = mutated("removeBatch", lambda: eng.removeBatch(gone))
    assert not set(gone.tolist()) & set(got[0].tolist())

    # five distinct predicates in flight: four entries, the fifth ticket is deferred
    preds = [{"denyFlags": bit}, {"timeRange": (100, None)}, {"timeRange": (None, 2_500)}, {"denyFlags": bit, "timeRange": (50, 2_900)}, {"timeRange": (7, 2_000)}]
    refs = [eng.searchFiltered(q, k, **p) for p in preds]
    before = s.stats()
    tickets = [eng.submitFiltered(q, k, **p) for p in preds]
    mid = s.delta(before)
    got = [eng.collect(t, k) for t in tickets]
    for i in range(5):
        assert_same(got[i], refs[i], f"five predicates, ticket {i}")
    assert mid["deferred"] == 1 and mid["rode"] == 4 and mid["masked_passes"] == 1, mid
    eng.close()


# ---- 7. a store without attributes ---------------------------------------------------------------------------------------------------------

def test_a_store_without_attributes_decides_on_the_host(wax):
    s = Store(wax, 0, R.store_rows("cos768"), attributes=False)
    eng, q = s.eng, s.queries[2]
    warm_code_mirror(eng, q)
    ref = eng.searchArrays(q, 10)
    before, passes = s.stats(), eng.getTuning("mirror_passes")
    got = eng.collect(eng.submitFiltered(q, 10, denyFlags=0b111), 10)
    d = s.delta(before)
    assert_same(got, ref, "denyFlags on a store without attributes")
    assert d["host_decided"] == 1 and d["submitted"] == 1 and d["rode"] == 0 and d["deferred"] == 0 and d["masked_passes"] == 0, d
    assert eng.getTuning("mirror_passes") == passes + 1               # the ticket's unmasked ride
    before, passes, searches = s.stats(), eng.getTuning("mirror_passes"), eng.stats().searches
    got = eng.collect(eng.submitFiltered(q, 10, timeRange=(1, None)), 10)
    d = s.delta(before)
    assert d["host_decided"] == 1 and d["rode"] == 0 and d["deferred"] == 0, d
    assert eng.getTuning("mirror_passes") == passes and eng.stats().searches == searches
    assert len(got[0]) == 0 and len(eng.searchFiltered(q, 10, timeRange=(1, None))[0]) == 0
    eng.close()


# ---- 8. edges of the ticket contract --------------------------------------------------------------------------------------------------------

def test_the_score_cut_threads_writers_and_the_empty_predicate(wax, stores):
    s = stores("cos384")
    eng, q, pred = s.eng, s.queries[9], predicate_of(s.n, "half")
    full = eng.searchFiltered(q, 10, **pred)
    cut = float(full[1][4])
    got = eng.collect(eng.submitFiltered(q, 10, minScore=cut, **pred), 10)
    assert_same(got, eng.searchFiltered(q, 10, minScore=cut, **pred), "score cut")
    assert len(got[0]) == 5
    assert_same(eng.collect(eng.submitFiltered(q, 10, minScore=float("nan"), **pred), 10), full, "a NaN cut keeps everything")
    # collected by another thread
    t = eng.submitFiltered(q, 10, **pred)
    box = {}
    th = threading.Thread(target=lambda: box.update(got=eng.collect(t, 10)))
    th.start()
    th.join()
    assert_same(box["got"], full, "collected from another thread")
    # a writer on the thread that holds a predicate ticket is refused
    t = eng.submitFiltered(q, 10, **pred)
    with pytest.raises(wax.WaxError, match="collect outstanding search tickets first"):
        eng.setAttributes([int(s.ids[0])], flags=[0])
    with pytest.raises(wax.WaxError, match="collect outstanding search tickets first"):
        eng.add(123456789, s.rows[0])
    assert_same(eng.collect(t, 10), full, "after the refused writers")
    # an empty predicate is wax_hip_search_submit (plus the cut)
    before = s.stats()
    plain = eng.searchArrays(q, 10)
    assert_same(eng.collect(eng.submitFiltered(q, 10), 10), plain, "empty predicate")
    got = eng.collect(eng.submitFiltered(q, 10, minScore=float(plain[1][2]), timeRange=(None, None), denyFlags=0), 10)
    assert_same(got, (plain[0][:3], plain[1][:3]), "empty predicate with a cut")
    assert s.delta(before) == {k: 0 for k in STAT_KEYS}


def test_existing_calls_leave_the_new_counters_at_zero(wax):
    rows, fl = R.store_rows("cos768"), flags_of(3_001, 768)
    s = Store(wax, 0, rows, fl)
    eng, bit = s.eng, R.MASK_BIT["half"]
    warm_code_mirror(eng, s.queries[0])
    tickets = [eng.submit(s.queries[i], 10) for i in range(6)]
    for t in tickets:
        eng.collect(t, 10)
    eng.searchFiltered(s.queries[0], 10, denyFlags=bit)
    eng.searchFiltered(s.queries[0], 10, frameIds=s.ids[:100], timeRange=(5, 2_000))
    eng.searchBatchFiltered(s.queries[:4], 10, denyFlags=bit)
    wax.searchManyFiltered([eng, eng], s.queries[:2], 10, denyFlags=bit)
    assert s.stats() == {k: 0 for k in STAT_KEYS}
    eng.close()
