"""The masked scan's mirror form ("predicate_mirror" 2): mirror_scan_masked_kernel + mirror_finish_kernel under the
row bitmap of a predicate search, and the host route around them.

Every answer is compared array_equal (ids and scores) with three references on the same engine: the same call under
"predicate_route" 1 (gather), the same call under "predicate_mirror" 0 with "predicate_route" 2 (the masked f32 scan), and
searchFiltered(frameIds = the passing ids). The iid cases are also held to the oracle under helpers.assert_parity. The counters say
which form answered: zero fallbacks are asserted exactly where tests/test_predicate_mirror_cpu.py has shown the certificate's margin
(or where this file computes it with the same model for a store it has just mutated), a fallback per query where the model's margin
is negative. Stores, masks and the model: predicate_mirror_ref.py."""
import numpy as np
import pytest

import oracle
import predicate_mirror_ref as R
from helpers import assert_parity

pytestmark = pytest.mark.gpu

COUNTERS = ("predicate_searches", "predicate_gather_searches", "predicate_masked_scans", "predicate_mirror_scans",
            "predicate_mirror_fallbacks", "predicate_mirror_unavailable")
CERTIFIED, FALLBACK, MASKED_F32, GATHER, NOTHING = [1, 0, 1, 1, 0, 0], [1, 0, 1, 0, 1, 0], [1, 0, 1, 0, 0, 0], [1, 1, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0]


@pytest.fixture(scope="module")
def wax(hip_lib):
    import wax_amd
    if hip_lib.wax_hip_device_count() == 0:
        pytest.skip("no HIP device on this host: the gpu-marked tests run on the MI355X box (pytest -m gpu)")
    assert hip_lib.wax_hip_available() == 1, "a HIP device is visible but it is not gfx950: the HIP path needs an MI355X"
    return wax_amd


class Store:
    """An engine over rows with ts = row and a flag column (a row fails a mask iff the mask's bit is set)."""

    def __init__(self, wax, metric, rows, flags, mirror=2, **kw):
        self.metric, (self.n, self.dims) = metric, rows.shape
        self.rows, self.fl = np.array(rows), np.array(flags, dtype=np.uint32)
        self.ids = np.arange(self.n, dtype=np.uint64) * 3 + 7
        self.ts = np.arange(self.n, dtype=np.int64)
        self.eng = wax.HIPVectorEngine(metric=wax.VectorMetric(metric), dimensions=self.dims, **kw)
        if kw.get("devices"):
            self.eng.setTuning("shard_min_mb", 0)
        self.eng.addBatch(self.ids, self.rows)
        assert self.eng.setAttributes(self.ids, self.ts, self.fl) == self.n
        if mirror is not None:
            self.eng.setTuning("predicate_mirror", mirror)
        self.queries = R.queries(self.dims)

    def counters(self):
        return [self.eng.getTuning(c) for c in COUNTERS]

    def passing(self, timeRange=None, denyFlags=0):
        m = (self.fl & np.uint32(denyFlags)) == 0
        if timeRange is not None:
            m &= (self.ts >= timeRange[0]) & (self.ts < timeRange[1])
        return m


@pytest.fixture(scope="module")
def stores(wax):
    made = {}

    def get(name):
        if name not in made:
            metric, n, dims = R.STORES[name]
            made[name] = Store(wax, metric, R.store_rows(name), R.flags_for(n, dims))
        return made[name]

    yield get
    for s in made.values():
        s.eng.close()


def predicate_of(s, mask_name):
    if mask_name == "range":
        return {"timeRange": R.range_bounds(s.n)}
    return {"denyFlags": R.MASK_BIT[mask_name]}


def check(s, k, q, expect, allow=None, parity=False, ctx="", **pred):
    """The mirror form against the three references; its counters against `expect`. `q`: an index into s.queries, or the query itself.
    Returns (ids, scores)."""
    eng, query = s.eng, (s.queries[q] if np.ndim(q) == 0 else q)
    mask = s.passing(**pred)
    if allow is not None:
        mask = mask & np.isin(s.ids, np.asarray(allow, dtype=np.uint64))
    eng.setTuning("predicate_route", 2)
    before = s.counters()
    got = eng.searchFiltered(query, k, frameIds=allow, **pred)
    delta = [a - b for a, b in zip(s.counters(), before)]
    assert delta == expect, f"{ctx}: counters {dict(zip(COUNTERS, delta))}"
    eng.setTuning("predicate_route", 1)
    gather = eng.searchFiltered(query, k, frameIds=allow, **pred)
    eng.setTuning("predicate_route", 2)
    eng.setTuning("predicate_mirror", 0)
    f32 = eng.searchFiltered(query, k, frameIds=allow, **pred)
    eng.setTuning("predicate_mirror", 2)
    eng.setTuning("predicate_route", 0)
    listed = eng.searchFiltered(query, k, frameIds=s.ids[mask])
    for ref, what in ((gather, "the gather route"), (f32, "the masked f32 scan"), (listed, "the allow-list of the passing ids")):
        assert np.array_equal(got[0], ref[0]), f"{ctx}: ids differ from {what}"
        assert np.array_equal(got[1], ref[1]), f"{ctx}: scores differ from {what}"
    assert len(got[0]) == min(k, int(mask.sum())), ctx
    if parity:
        rows = np.flatnonzero(mask)
        ei, es, _, _ = oracle.search(s.metric, s.rows[rows], s.ids[rows], query, k)
        _, es_all, _, _ = oracle.search(s.metric, s.rows[rows], s.ids[rows], query, min(k + 10, len(rows)))
        assert_parity(got[0], got[1], ei, es, all_exp_scores=es_all, ctx=ctx)
    return got


# ---- 1. every mask and top_k on the iid stores: certified, bit for bit the three references -----------------------------------------

@pytest.mark.parametrize("name", list(R.STORES))
def test_every_mask_and_top_k_is_certified_and_equal(stores, name):
    s = stores(name)
    ms = R.masks(s.n, s.dims)
    f0 = s.eng.getTuning("predicate_mirror_fallbacks")
    for mask_name in R.TAKEN_MASKS:
        pred = predicate_of(s, mask_name)
        assert np.array_equal(s.passing(**pred), ms[mask_name])
        for k in R.KS:
            for q in (0, 1, 2):
                check(s, k, q, CERTIFIED, parity=(k == 10 and q == 0), ctx=f"{name} {mask_name} top_k {k} query {q}", **pred)
    assert s.eng.getTuning("predicate_mirror_fallbacks") == f0 and s.eng.getTuning("predicate_mirror_unavailable") == 0


@pytest.mark.parametrize("name", ["cos384", "dot768"])
def test_64_or_fewer_passing_rows_and_top_k_33_are_not_taken(stores, name):
    s = stores(name)
    assert s.passing(**predicate_of(s, "m65")).sum() == 65 and s.passing(**predicate_of(s, "m64")).sum() == 64
    check(s, 10, 3, CERTIFIED, ctx="65 rows pass: the smallest taken", **predicate_of(s, "m65"))
    check(s, 32, 3, CERTIFIED, ctx="65 rows pass, top_k 32", **predicate_of(s, "m65"))
    check(s, 10, 3, MASKED_F32, ctx="64 rows pass", **predicate_of(s, "m64"))
    check(s, 10, 3, NOTHING, ctx="no row passes", **predicate_of(s, "m0"))
    check(s, 33, 3, MASKED_F32, ctx="top_k 33", **predicate_of(s, "half"))
    check(s, 100, 3, MASKED_F32, ctx="top_k 100", **predicate_of(s, "r15"))


def test_l2_and_generic_dimensions_are_not_taken(wax):
    rows = R.store_rows("cos384")[:3_001]
    fl = R.flags_for(20_005, 384)[:3_001]
    s = Store(wax, 2, rows, fl)
    check(s, 10, 0, MASKED_F32, ctx="L2", denyFlags=R.MASK_BIT["half"])
    s.eng.close()
    s = Store(wax, 0, np.ascontiguousarray(rows[:, :100]), fl)
    check(s, 10, 0, GATHER, ctx="100-d", denyFlags=R.MASK_BIT["half"])
    s.eng.close()


def test_an_allow_list_is_anded_in(stores):
    s = stores("cos384")
    rng = np.random.default_rng(11)
    allow = np.concatenate([s.ids[rng.choice(s.n, 9_000, replace=False)], np.arange(10 ** 9, 10 ** 9 + 40, dtype=np.uint64)])
    assert len(allow) >= 4096
    for mask_name in ("half", "range"):
        pred = predicate_of(s, mask_name)
        both = s.passing(**pred) & np.isin(s.ids, allow)
        for k, q in ((10, 4), (32, 5)):
            assert R.model("cos384").margin(both, q, k) > R.MARGIN_FLOOR
            check(s, k, q, CERTIFIED, allow=allow, parity=(k == 10), ctx=f"{mask_name} and an allow-list of {len(allow)}", **pred)


# ---- 2. statistics -----------------------------------------------------------------------------------------------------------------

def live_chunks(mask, c):
    return int(np.count_nonzero(np.add.reduceat(mask.astype(np.int64), np.arange(0, len(mask), c))))


@pytest.mark.parametrize("name", ["cos384", "cos768"])
def test_bytes_and_skipped_chunks_are_the_mirrors(stores, name):
    s = stores(name)
    c, eng = R.MIRROR_CHUNK[s.dims], s.eng
    n_chunks = -(-s.n // c)
    for mask_name in ("range", "one_per_chunk", "tail_plus_65"):
        pred = predicate_of(s, mask_name)
        live = live_chunks(s.passing(**pred), c)
        eng.setTuning("predicate_route", 2)
        st0, k0, m0 = eng.stats(), eng.getTuning("predicate_chunks_skipped"), eng.getTuning("predicate_mirror_scans")
        eng.searchFiltered(s.queries[0], 10, **pred)
        eng.setTuning("predicate_route", 0)
        st1 = eng.stats()
        assert eng.getTuning("predicate_mirror_scans") == m0 + 1
        assert st1.searches - st0.searches == 1
        assert st1.bytes_scanned - st0.bytes_scanned == live * c * s.dims * 2 + R.MIRROR_KP * s.dims * 4, mask_name
        assert eng.getTuning("predicate_chunks_skipped") - k0 == n_chunks - live, mask_name
    assert live_chunks(s.passing(**predicate_of(s, "one_per_chunk")), c) == n_chunks


# ---- 3. exact duplicates: every query falls back, the answers stay -------------------------------------------------------------------

def test_duplicate_store_falls_back_every_time(wax):
    s = Store(wax, 0, R.dup_rows(), np.zeros(R.DUP_ROWS, dtype=np.uint32))
    tr = (0, R.DUP_PASSING)
    assert np.array_equal(s.passing(timeRange=tr), R.dup_mask())
    eng, c, c32 = s.eng, R.MIRROR_CHUNK[s.dims], R.F32_CHUNK[s.dims]
    # what the masked f32 scan reports when taken directly
    eng.setTuning("predicate_route", 2)
    eng.setTuning("predicate_mirror", 0)
    st0, k0 = eng.stats(), eng.getTuning("predicate_chunks_skipped")
    eng.searchFiltered(s.queries[0], 10, timeRange=tr)
    direct_bytes, direct_skipped = eng.stats().bytes_scanned - st0.bytes_scanned, eng.getTuning("predicate_chunks_skipped") - k0
    assert direct_bytes == live_chunks(R.dup_mask(), c32) * c32 * s.dims * 4
    eng.setTuning("predicate_mirror", 2)
    for k in R.KS:
        for q in (0, 1, 2):
            got = check(s, k, q, FALLBACK, ctx=f"duplicates top_k {k} query {q}", timeRange=tr)   # once in "predicate_masked_scans"
            assert list(got[0]) == sorted(got[0]) and len(set(got[1].tolist())) == 1, "70 equal best rows, in ascending row order"
    eng.close()
    # the fallback's figures are the mirror pass's plus the f32 route's own
    s = Store(wax, 0, R.dup_rows(), np.zeros(R.DUP_ROWS, dtype=np.uint32))
    eng = s.eng
    eng.setTuning("predicate_route", 2)
    st0, k0 = eng.stats(), eng.getTuning("predicate_chunks_skipped")
    eng.searchFiltered(s.queries[0], 10, timeRange=tr)
    st1 = eng.stats()
    live = live_chunks(R.dup_mask(), c)
    assert eng.getTuning("predicate_mirror_fallbacks") == 1 and st1.searches - st0.searches == 1
    assert st1.bytes_scanned - st0.bytes_scanned == live * c * s.dims * 2 + R.MIRROR_KP * s.dims * 4 + direct_bytes
    assert eng.getTuning("predicate_chunks_skipped") - k0 == (-(-s.n // c) - live) + direct_skipped
    eng.close()


# ---- 4. the mirror follows the store row by row ----------------------------------------------------------------------------------------

def test_the_mirror_follows_appends_upserts_and_removals(wax):
    dims, bit = 384, 1 << 8
    pool = oracle.gaussian_unit_rows(0, 4_000, dims, seed=R.STORE_SEED + 3)
    rng = np.random.default_rng(5)
    fl_pool = np.where(rng.random(4_000) < 0.5, bit, 0).astype(np.uint32)
    s = Store(wax, 0, pool[:3_001], fl_pool[:3_001])
    eng, q = s.eng, s.queries[6]

    def verify(ctx, top=None):
        s.n = len(s.ids)
        s.ts = np.array(eng.getAttributes(s.ids)[0])
        model = R.Model(0, s.rows, q[None, :])                 # the store as it is now: the margin before the counters are held to it
        for k in (10, 32):
            assert model.margin(s.passing(denyFlags=bit), 0, k) > R.MARGIN_FLOOR, ctx
            got = check(s, k, q, CERTIFIED, parity=(k == 10), ctx=ctx, denyFlags=bit)
        if top is not None:
            assert int(got[0][0]) == top, ctx
        return got

    first = verify("as built")
    c0 = eng.getTuning("mirror_conversions")
    # append: rows of the pool, one of them the query itself (it passes: flags 0)
    new_rows = pool[3_001:3_500].copy()
    new_rows[17] = q
    new_fl = fl_pool[3_001:3_500].copy()
    new_fl[17] = 0
    new_ids = np.arange(10 ** 6, 10 ** 6 + len(new_rows), dtype=np.uint64)
    eng.addBatch(new_ids, new_rows)
    assert eng.setAttributes(new_ids, np.arange(len(new_ids)) + 50_000, new_fl) == len(new_ids)
    s.rows, s.ids, s.fl = np.concatenate([s.rows, new_rows]), np.concatenate([s.ids, new_ids]), np.concatenate([s.fl, new_fl])
    verify("after an append", top=10 ** 6 + 17)
    assert eng.getTuning("mirror_conversions") == c0 + 1, "the append converted its own rows"
    # upsert: the appended best row becomes an ordinary one, an old passing row becomes the best
    old = int(np.flatnonzero(s.passing(denyFlags=bit))[40])
    eng.add(int(new_ids[17]), pool[3_600])
    eng.add(int(s.ids[old]), q)
    s.rows[3_001 + 17], s.rows[old] = pool[3_600], q
    verify("after two upserts", top=int(s.ids[old]))
    # remove the best row: yesterday's answer without it
    eng.remove(int(s.ids[old]))
    keep = np.arange(len(s.ids)) != old
    s.rows, s.ids, s.fl = s.rows[keep], s.ids[keep], s.fl[keep]
    got = verify("after remove")
    assert int(s.ids[old]) not in got[0].tolist()
    # removeBatch: the ten best passing rows and a run in the middle
    gone = np.concatenate([got[0][:10], s.ids[1_000:1_300]])
    assert eng.removeBatch(gone) == len(set(gone.tolist()))
    keep = ~np.isin(s.ids, gone)
    s.rows, s.ids, s.fl = s.rows[keep], s.ids[keep], s.fl[keep]
    got = verify("after removeBatch")
    assert not set(gone.tolist()) & set(got[0].tolist()) and len(first[0]) == 32
    assert eng.getTuning("predicate_mirror_fallbacks") == 0 and eng.getTuning("predicate_mirror_unavailable") == 0
    eng.close()


# ---- 5. the batched call's leftover queries and a sharded handle inherit the form --------------------------------------------------

def test_batched_predicate_queries_that_loop_take_the_form(stores):
    s = stores("cos384")
    eng, bit = s.eng, R.MASK_BIT["half"]
    singles = [check(s, 10, q, CERTIFIED, ctx=f"single {q}", denyFlags=bit) for q in (0, 1, 2)]
    eng.setTuning("predicate_route", 2)
    eng.setTuning("filter_batch", 0)
    try:
        m0 = eng.getTuning("predicate_mirror_scans")
        ids, scores, counts = eng.searchBatchFiltered(s.queries[:3], 10, denyFlags=bit)
        assert eng.getTuning("predicate_mirror_scans") == m0 + 3
    finally:
        eng.setTuning("filter_batch", 1)
        eng.setTuning("predicate_route", 0)
    for i in range(3):
        assert counts[i] == 10 and np.array_equal(ids[i, :10], singles[i][0]) and np.array_equal(scores[i, :10], singles[i][1])


def test_two_shards_on_one_device_give_the_same_answers(wax, stores):
    one = stores("cos768")
    many = Store(wax, 0, one.rows, one.fl, devices=[0, 0])
    assert many.eng.getTuning("shards") == 2 and many.eng.getTuning("predicate_mirror") == 2
    for mask_name in ("r15", "range", "one_per_chunk"):
        pred = predicate_of(one, mask_name)
        for k, q in ((1, 7), (10, 8), (32, 9)):
            before = many.counters()
            many.eng.setTuning("predicate_route", 2)
            b = many.eng.searchFiltered(one.queries[q], k, **pred)
            many.eng.setTuning("predicate_route", 0)
            delta = [x - y for x, y in zip(many.counters(), before)]
            a = check(one, k, q, CERTIFIED, ctx=f"single engine {mask_name} {k}", **pred)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), f"{mask_name} top_k {k}"
            # every shard that holds passing rows answers; counters are summed over the shards
            assert delta[0] == 2 and delta[1] == 0 and delta[2] == delta[3] + delta[4] >= 1 and delta[5] == 0, delta
    many.eng.close()


# ---- 6. the key ------------------------------------------------------------------------------------------------------------------------

def test_the_key_its_default_and_what_a_small_store_does_under_it(wax):
    rows, fl = R.store_rows("cos384")[:3_001], R.flags_for(20_005, 384)[:3_001]
    s = Store(wax, 0, rows, fl, mirror=None)
    eng, bit, c32 = s.eng, R.MASK_BIT["half"], R.F32_CHUNK[384]
    assert eng.getTuning("predicate_mirror") == 1
    for bad in (3, -1):
        with pytest.raises(wax.EncodingError, match="predicate_mirror"):
            eng.setTuning("predicate_mirror", bad)
    assert eng.getTuning("predicate_mirror") == 1
    # auto on a store far below 2 GiB: today's masked f32 scan, today's figures, no mirror built
    eng.setTuning("predicate_route", 2)
    before, st0, k0 = s.counters(), eng.stats(), eng.getTuning("predicate_chunks_skipped")
    got = eng.searchFiltered(s.queries[0], 10, denyFlags=bit)
    assert [a - b for a, b in zip(s.counters(), before)] == MASKED_F32
    live = live_chunks(s.passing(denyFlags=bit), c32)
    assert eng.stats().bytes_scanned - st0.bytes_scanned == live * c32 * 384 * 4
    assert eng.getTuning("predicate_chunks_skipped") - k0 == -(-s.n // c32) - live
    assert eng.getTuning("mirror_conversions") == 0
    for mode, expect in ((2, CERTIFIED), (0, MASKED_F32), (1, MASKED_F32)):
        eng.setTuning("predicate_mirror", mode)
        assert eng.getTuning("predicate_mirror") == mode
        before = s.counters()
        again = eng.searchFiltered(s.queries[0], 10, denyFlags=bit)
        assert [a - b for a, b in zip(s.counters(), before)] == expect, mode
        assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1])
    # "scan_mirror" 0 switches the auto mode off, not the forced one; "force_general" and a kernel variant keep the f32 forms
    eng.setTuning("predicate_mirror", 2)
    for key, value, expect in (("scan_mirror", 0, CERTIFIED), ("force_general", 1, GATHER), ("variant", 1, MASKED_F32), ("grid_blocks", 1024, MASKED_F32)):
        old = eng.getTuning(key)
        eng.setTuning(key, value)
        before = s.counters()
        again = eng.searchFiltered(s.queries[0], 10, denyFlags=bit)
        eng.setTuning(key, old)
        assert [a - b for a, b in zip(s.counters(), before)] == expect, key
        assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1]), key
    eng.close()
