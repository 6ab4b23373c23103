"""The required-term search on the device (wax_amd/csrc/terms.hip; wax_hip_search_terms / _set_terms / _term_mask_probe) against the
restatement of its contract in tests/terms_ref.py. Every comparison is array_equal: the probe's bitmap against the numpy bitmap, an
engine's answer against searchFiltered(frameIds = the ids the model passes) on the same engine — ids and score bits.

The mask has two forms (wax_amd/csrc/terms.hip): the product's lane-per-row kernel and the wave-cooperative one a build with
-DWAX_TERM_MASK_FORM=0 launches in its place; the same cases hold both. The wave form consumes a wave's span in pieces of
ref.PIECE = 1 024 values (TERM_MASK_PIECE), so its loop has boundaries at 1 024, 2 048 and 3 072 values from the 16-byte boundary below
the span's start. The shapes "straddle", "straddle2" and "straddle3" put 17 .. 19, 33 .. 35 and 49 .. 51 terms in every row: a
wave's span is about 1 150, 2 180 and 3 200 values, and the test asserts that a SET lies across every boundary up to the shape's
last, across that one in waves that start at every residue of 4 (at 4 097 and 20 000 rows). The all-64 shape makes a span four
pieces long with every boundary between two sets — and is the lane-per-row form's longest loop in every lane; "one64" and "gaps" are
its most divergent waves."""
import numpy as np
import pytest

import terms_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def wax():
    import wax_amd
    if not wax_amd.HIPVectorEngine.isAvailable():
        pytest.skip("no gfx950 device")
    return wax_amd


# ---- through the probe ------------------------------------------------------------------------------------------------------

ROWS = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 4097, 20_000)
GRIDS = (1, 2, 3)
SHAPES = ("empty", "gaps", "all64", "one64", "straddle", "straddle2", "straddle3", "random")


def shape_lens(shape, n, rng):
    """(terms per row, which rows hold COMMON)"""
    r = np.arange(n)
    if shape == "empty":
        return np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    if shape == "gaps":                                          # empty rows between full ones
        full = r % 3 == 0
        return np.where(full, 64, 0), full.astype(np.int64)
    if shape == "all64":                                         # one wave's span is 4 096 values: four pieces
        return np.full(n, 64), np.ones(n, dtype=np.int64)
    if shape == "one64":                                         # one 64-term row among empty ones
        one = r == n // 2
        return np.where(one, 64, 0), one.astype(np.int64)
    if shape in STRADDLE:                                        # 64 rows x (base .. base + 2) terms: just over 1, 2, 3 pieces of ref.PIECE
        base, pieces = STRADDLE[shape]
        assert 64 * (base - 1) <= pieces * ref.PIECE < 64 * base
        return base + r % 7 % 3, np.ones(n, dtype=np.int64)           # (r % 7 % 3: the waves' spans then start at every residue of 4)
    return rng.integers(0, 65, size=n), (rng.random(n) < 0.5).astype(np.int64)


STRADDLE = {"straddle": (17, 1), "straddle2": (33, 2), "straddle3": (49, 3)}   # shape -> (fewest terms per row, piece boundaries crossed)


def straddled(off, boundary):
    """Per full wave (64 rows) of a column: does one SET lie across `boundary` values, counted as the kernel's loop counts them — from
    the 16-byte boundary at or below the wave's first value? Returns (waves where one does, the `lead` residues of those waves)."""
    off = off.astype(np.int64)
    waves, leads = 0, set()
    for r0 in range(0, len(off) - 1 - 63, 64):
        lead = int(off[r0] & 3)
        rel = off[r0:r0 + 65] - off[r0] + lead
        if bool(((rel[:-1] < boundary) & (rel[1:] > boundary)).any()):
            waves += 1
            leads.add(lead)
    return waves, leads


def special_counts(kind, n, rng):
    """How many of ref.SPECIALS each row holds (its first c): who passes a requirement of SPECIALS[:m] is who has c >= m."""
    c = np.zeros(n, dtype=np.int64)
    if kind == "row0":
        c[0] = 16
    elif kind == "last":
        c[n - 1] = 16
    elif kind == "last_word":                                    # passing rows only in the final, partial bitmap word
        c[(n - 1) // 32 * 32:] = 16
    elif kind == "mixed":
        c = np.where(rng.random(n) < 0.4, rng.integers(1, 17, size=n), 0)
        c[rng.integers(0, n)] = 16
    return c


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("n", ROWS)
def test_probe_equals_the_numpy_bitmap(wax, n, shape):
    rng = np.random.default_rng(n * 131 + len(shape))
    lens, common = shape_lens(shape, n, rng)
    bitmap_in = rng.integers(0, 2**32, size=(n + 31) // 32, dtype=np.uint64).astype(np.uint32)
    all16 = [int(t) for t in ref.SPECIALS]
    passed = 0
    for kind in ("none", "row0", "last", "last_word", "mixed"):
        off, val = ref.build_column(lens, special_counts(kind, n, rng), common)
        if shape in STRADDLE and n >= 4097:
            # a set lies across EVERY piece boundary up to the one the shape is named for, in at least half of the waves; across that
            # last one in waves whose span starts at every residue of 4 (the lower boundaries have that from the shapes named for them)
            last = STRADDLE[shape][1]
            for b in range(1, last + 1):
                waves, leads = straddled(off, b * ref.PIECE)
                assert waves >= (n // 64) // 2 and (b < last or leads == {0, 1, 2, 3}), (shape, kind, b, waves, leads)
        if kind == "none":
            reqs = ([ref.NOBODY], [ref.COMMON], [ref.COMMON, ref.NOBODY])       # a term nobody holds, one everybody (of this shape) holds
        elif kind == "mixed":
            reqs = ([1], [2, 1], all16, [16], [ref.COMMON, 3], all16 + [1, 16])   # 1, 2 and 16 required terms; duplicates collapse
        else:
            reqs = (all16, [1, 2], [7])
        for req in reqs:
            want = ref.pass_csr(off, val, req)
            passed += int(want.sum())
            for bm in (None, bitmap_in):
                exp = ref.bitmap_of(want if bm is None else want & ref.bits_of(bm, n))
                for grid in GRIDS:
                    got = wax.termMaskProbe(off, val, req, bitmapIn=bm, grid=grid)
                    assert np.array_equal(got, exp), (kind, req, bm is not None, grid)
    assert passed > 0


def test_probe_model_places_the_only_passing_row_where_the_case_says(wax):
    """The cases above are what they claim to be: one passing row at row 0 / at the last row, rows of the final word only."""
    n = 4097
    rng = np.random.default_rng(5)
    lens, common = shape_lens("random", n, rng)
    for kind, rows in (("row0", [0]), ("last", [n - 1]), ("last_word", [4096])):
        off, val = ref.build_column(lens, special_counts(kind, n, rng), common)
        assert np.nonzero(ref.pass_csr(off, val, ref.SPECIALS))[0].tolist() == rows
        assert ref.bits_of(wax.termMaskProbe(off, val, ref.SPECIALS, grid=2), n).nonzero()[0].tolist() == rows


# ---- through an engine ------------------------------------------------------------------------------------------------------

METRICS = ("cosine", "dot", "l2")
SESSION0, TAG0, EVERYBODY, NOBODY = 1000, 2000, 7, 8


def corpus(n, dims, seed):
    """Gaussian rows of which about a sixth repeat an earlier row bit for bit: equal scores, decided by row order."""
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((n, dims)).astype(np.float32)
    dup = np.nonzero(rng.random(n) < 0.17)[0]
    dup = dup[dup > 0]
    rows[dup] = rows[rng.integers(0, dup)]
    return rows, rng.standard_normal((3, dims)).astype(np.float32)


def term_sets(n, seed, sessions=2):
    """Six terms per row: a session id, two tags of four, EVERYBODY, two private ones."""
    rng = np.random.default_rng(seed)
    ses = rng.integers(0, sessions, size=n)
    t1, t2 = rng.integers(0, 4, size=n), rng.integers(0, 4, size=n)
    return [(SESSION0 + int(ses[r]), TAG0 + int(t1[r]), TAG0 + 10 + int(t2[r]), EVERYBODY, 100_000 + 2 * r, 100_001 + 2 * r) for r in range(n)]


class Store:
    def __init__(self, wax, metric, n, dims, seed, devices=None, sessions=2):
        from wax_amd import VectorMetric
        self.n, self.dims = n, dims
        self.rows, self.queries = corpus(n, dims, seed)
        self.fids = np.random.default_rng(seed + 1).permutation(n).astype(np.uint64) * 3 + 5
        self.sets = term_sets(n, seed + 2, sessions)
        self.ts = np.random.default_rng(seed + 3).integers(0, 100, size=n).astype(np.int64)
        self.fl = np.where(np.random.default_rng(seed + 4).random(n) < 0.2, 0x100, 0).astype(np.uint32)
        self.eng = wax.HIPVectorEngine(metric=getattr(VectorMetric, metric), dimensions=dims, devices=devices)
        if devices:
            self.eng.setTuning("shard_min_mb", 0)
            self.eng.reserve(n)
        self.eng.addBatch(self.fids, self.rows)
        assert self.eng.setTerms(self.fids, self.sets) == n
        assert self.eng.setAttributes(self.fids, self.ts, self.fl) == n

    def check(self, req, k=10, q=0, frameIds=None, expect_some=True, **filters):
        """searchFiltered(requiredTerms=req) == searchFiltered(frameIds = what the model passes [and the caller allows])."""
        eng, query = self.eng, self.queries[q]
        passing = ref.pass_set(self.sets, req)
        ids = self.fids[passing]
        if frameIds is not None:
            ids = ids[np.isin(ids, frameIds)]
        exp = eng.searchFiltered(query, k, frameIds=ids, **filters)
        got = eng.searchFiltered(query, k, frameIds=frameIds, requiredTerms=req, **filters)
        what = (self.n, req, k, q, filters)
        assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1].view(np.int32), exp[1].view(np.int32)), what
        if expect_some:
            # neither a filter that does nothing nor one that drops everything nor a silent fall-back to the unfiltered search
            plain = eng.searchFiltered(query, k, frameIds=frameIds, **filters)
            differs = not np.array_equal(got[0], plain[0])
            assert passing.any() and not passing.all() and len(got[0]) > 0, what
            assert differs == bool(np.isin(plain[0], self.fids[~passing]).any()), what   # exactly when the unfiltered answer holds a failing row
            assert differs or k < 10, what                                              # (which ten results always do here; one result may not)
        return got


@pytest.fixture(scope="module")
def stores(wax):
    made = {}

    def get(metric, n, dims=384):
        key = (metric, n, dims)
        if key not in made:
            made[key] = Store(wax, metric, n, dims, seed=n + dims + len(metric))
        return made[key]
    yield get
    for s in made.values():
        s.eng.close()


REQS = ([SESSION0], [SESSION0 + 1, TAG0 + 2], [TAG0 + 1, TAG0 + 13, EVERYBODY, SESSION0])


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n", (257, 4097, 9999))
def test_every_route_answers_as_the_allow_list_of_the_passing_rows(stores, n, metric):
    s = stores(metric, n)
    eng = s.eng
    try:
        for route, mirror, counter in ((1, 0, "predicate_gather_searches"), (2, 0, "predicate_masked_scans"), (2, 2, "predicate_mirror_scans")):
            eng.setTuning("predicate_route", route)
            eng.setTuning("predicate_mirror", mirror)
            # (the mirror form needs more than 64 passing rows: the two sessions, each against every query)
            cases = [(qi, [SESSION0 + ses]) for ses in (0, 1) for qi in range(3)] if mirror else list(enumerate(REQS))
            certified = 0
            for qi, req in cases:
                t0, c0 = eng.termStats(), eng.getTuning(counter)
                f0, u0 = eng.getTuning("predicate_mirror_fallbacks"), eng.getTuning("predicate_mirror_unavailable")
                p0, m0 = eng.getTuning("predicate_searches"), eng.getTuning("predicate_masked_scans")
                got = eng.searchFiltered(s.queries[qi], 10, requiredTerms=req)
                t1 = eng.termStats()
                assert t1["device_masks"] == t0["device_masks"] + 1 and t1["searches"] == t0["searches"] + 1
                assert t1["host_staged"] == t0["host_staged"] and t1["host_decided"] == t0["host_decided"]
                assert eng.getTuning("predicate_searches") == p0 + 1
                if mirror and metric == "l2":                                   # (no bf16 mirror under l2: the masked f32 scan)
                    assert eng.getTuning("predicate_masked_scans") == m0 + 1 and eng.getTuning(counter) == c0
                elif mirror:
                    # the certificate released the answer, or the masked f32 scan gave it on the same bitmap: never the gather
                    assert int(ref.pass_set(s.sets, req).sum()) > 64
                    fell = eng.getTuning("predicate_mirror_fallbacks") - f0
                    assert eng.getTuning(counter) - c0 + fell == 1 and eng.getTuning("predicate_mirror_unavailable") == u0
                    certified += eng.getTuning(counter) - c0
                else:
                    assert eng.getTuning(counter) == c0 + 1
                chk = s.check(req, 10, qi)
                assert np.array_equal(chk[0], got[0]) and np.array_equal(chk[1], got[1])
            if mirror and metric != "l2":
                assert certified >= 1, (n, metric, certified)                   # the certificate did release answers: not six fallbacks
            for k in (1, 33):
                s.check(REQS[1], k, 2)
    finally:
        eng.setTuning("predicate_route", 0)
        eng.setTuning("predicate_mirror", 1)


def test_a_dimension_outside_the_lane_shape_table_gathers(stores):
    s = stores("cosine", 1500, 20)
    g0 = s.eng.getTuning("predicate_gather_searches")
    s.eng.setTuning("predicate_route", 2)
    try:
        for qi, req in enumerate(REQS):
            s.check(req, 10, qi)
    finally:
        s.eng.setTuning("predicate_route", 0)
    assert s.eng.getTuning("predicate_gather_searches") > g0 and s.eng.termStats()["device_masks"] >= 3


@pytest.mark.parametrize("route", (1, 2))
def test_combined_with_the_other_filters(stores, route):
    s = stores("cosine", 9999)
    eng = s.eng
    eng.setTuning("predicate_route", route)
    try:
        m0 = eng.termStats()["device_masks"]
        s.check([SESSION0], 10, 0, timeRange=(20, 80))
        s.check([SESSION0, TAG0], 10, 1, denyFlags=0x100)
        s.check([SESSION0 + 1], 10, 2, timeRange=(None, 50), denyFlags=0x100)
        assert eng.termStats()["device_masks"] == m0 + 3
        # minScore: the cut on the host, behind the same selection
        got = s.check([SESSION0], 10, 0)
        cut = float(got[1][4])
        trimmed = s.check([SESSION0], 10, 0, minScore=cut)
        assert np.array_equal(trimmed[0], got[0][got[1] >= cut]) and len(trimmed[0]) >= 5
        # a short allow-list is staged on the host, where the term test reads the host column
        t0 = eng.termStats()
        short = s.fids[::7][:500]
        s.check([SESSION0], 10, 1, frameIds=short)
        s.check([SESSION0], 10, 1, frameIds=short, timeRange=(10, 90))
        t1 = eng.termStats()
        assert t1["host_staged"] == t0["host_staged"] + 2 and t1["device_masks"] == t0["device_masks"]
        # a list of at least "filter_device_min" ids: the probe marks the bitmap, the term mask ANDs into it
        assert eng.getTuning("filter_device_min") == 4096
        long_list = np.concatenate([s.fids[::2], np.array([2**40, 2**40 + 1], dtype=np.uint64)])
        assert len(long_list) >= 4096
        s.check([SESSION0], 10, 2, frameIds=long_list)
        s.check([SESSION0 + 1, TAG0 + 3], 10, 0, frameIds=long_list, denyFlags=0x100)
        t2 = eng.termStats()
        assert t2["device_masks"] == t1["device_masks"] + 2 and t2["host_staged"] == t1["host_staged"]
    finally:
        eng.setTuning("predicate_route", 0)


def test_degenerate_forms(wax, stores):
    s = stores("cosine", 4097)
    eng, q = s.eng, s.queries[0]
    # no required term: the predicate search's arrays, and no term search counted
    t0 = eng.termStats()
    for kw in ({}, {"timeRange": (10, 60)}, {"frameIds": s.fids[:300], "denyFlags": 0x100}):
        a, b = eng.searchFiltered(q, 10, requiredTerms=[], **kw), eng.searchFiltered(q, 10, **kw)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and len(a[0]) > 0
    assert eng.termStats() == t0
    # a term nobody holds; NO_MATCH without a call
    got = eng.searchFiltered(q, 10, requiredTerms=[NOBODY])
    assert len(got[0]) == 0 and eng.termStats()["device_masks"] == t0["device_masks"] + 1
    t1 = eng.termStats()
    assert len(eng.searchFiltered(q, 10, requiredTerms=wax.TermDictionary.NO_MATCH)[0]) == 0 and eng.termStats() == t1
    # too many distinct terms
    with pytest.raises(Exception, match="more than 16"):
        eng.searchFiltered(q, 10, requiredTerms=list(range(17)))
    assert len(eng.searchFiltered(q, 10, requiredTerms=[EVERYBODY] * 40)[0]) == 10      # duplicates collapse
    # terms never set: count 0, decided on the host
    bare = wax.HIPVectorEngine(dimensions=384)
    bare.addBatch(s.fids[:300], s.rows[:300])
    assert bare.getTerms(int(s.fids[0])).size == 0 and bare.getTerms(1) is None
    got = bare.searchFiltered(q, 10, requiredTerms=[EVERYBODY])
    st = bare.termStats()
    assert len(got[0]) == 0 and st["host_decided"] == 1 and st["device_masks"] == 0 and st["term_rows_uploaded"] == 0
    # set_terms: refusals leave everything as it was; getTerms returns the set ascending
    with pytest.raises(Exception, match="more than 64"):
        bare.setTerms(s.fids[:2], [[1], list(range(65))])
    assert bare.termStats()["host_decided"] == 1 and len(bare.searchFiltered(q, 10, requiredTerms=[1])[0]) == 0
    assert bare.termStats()["host_decided"] == 2
    assert bare.setTerms([int(s.fids[3]), 2, int(s.fids[3])], [[9, 9], [4], [6, 5, 6]]) == 2      # an unknown id is skipped; the last entry wins
    assert bare.getTerms(int(s.fids[3])).tolist() == [5, 6] and bare.getTerms(int(s.fids[4])).size == 0
    got = bare.searchFiltered(q, 10, requiredTerms=[6, 5])
    assert got[0].tolist() == [int(s.fids[3])] and bare.termStats()["device_masks"] == 1
    bare.close()


# ---- the column's lifecycle -------------------------------------------------------------------------------------------------

def fresh_answers(wax, model, reqs, queries, k=10):
    eng = wax.HIPVectorEngine(dimensions=model.dims)
    ids = np.asarray(model.ids, dtype=np.uint64)
    eng.addBatch(ids, model.matrix())
    if any(model.sets):
        eng.setTerms(ids, model.sets)
    out = [eng.searchFiltered(q, k, requiredTerms=req) for req in reqs for q in queries]
    eng.close()
    return out


def test_lifecycle_follows_the_other_columns(wax):
    dims = 64
    rng = np.random.default_rng(17)
    n0 = 600
    rows, queries = corpus(5000, dims, 23)
    fids = np.arange(5000, dtype=np.uint64) * 2 + 11
    sets = term_sets(5000, 29, sessions=3)
    reqs = ([SESSION0], [SESSION0 + 1, EVERYBODY], [TAG0 + 2])
    eng = wax.HIPVectorEngine(dimensions=dims)
    model = ref.StoreModel(dims)
    eng.addBatch(fids[:n0], rows[:n0])
    model.add_batch(fids[:n0], rows[:n0])
    eng.setTerms(fids[:n0], sets[:n0])
    model.set_terms(fids[:n0], sets[:n0])

    def same(lowest_changed, what):
        """The live engine answers as a fresh one built from the model; the upload covers at most the rows from the lowest change on."""
        u0 = eng.termStats()["term_rows_uploaded"]
        got = [eng.searchFiltered(q, 10, requiredTerms=req) for req in reqs for q in queries]
        exp = fresh_answers(wax, model, reqs, queries)
        for (gi, gs), (ei, es) in zip(got, exp):
            assert np.array_equal(gi, ei) and np.array_equal(gs.view(np.int32), es.view(np.int32)), what
        assert any(len(g[0]) for g in got) or not any(model.sets), what
        up = eng.termStats()["term_rows_uploaded"] - u0
        bound = 0 if lowest_changed is None else eng.count - lowest_changed
        assert up <= bound, (what, up, bound)
        for f in rng.choice(np.asarray(model.ids, dtype=np.uint64), 20):
            assert eng.getTerms(int(f)).tolist() == list(model.sets[model.ids.index(int(f))]), what

    same(0, "first upload")
    same(None, "nothing changed")
    # add: the new rows hold the empty set
    eng.add(int(fids[n0]), rows[n0]); model.add(fids[n0], rows[n0])
    same(n0, "add")
    # upsert: the row keeps its set
    eng.add(int(fids[5]), rows[4000]); model.add(fids[5], rows[4000])
    same(None, "upsert")
    # remove: the row's set goes with it
    eng.remove(int(fids[100])); model.remove(fids[100])
    same(100, "remove")
    gone = fids[[7, 300, 301, 599]]
    assert eng.removeBatch(gone) == 4
    model.remove_batch(gone)
    same(7, "removeBatch")
    # growth past capacity, then terms for some of the new rows
    before = eng.count
    eng.addBatch(fids[n0 + 1:4000], rows[n0 + 1:4000]); model.add_batch(fids[n0 + 1:4000], rows[n0 + 1:4000])
    same(before, "growth")
    eng.setTerms(fids[2000:3000], sets[2000:3000]); model.set_terms(fids[2000:3000], sets[2000:3000])
    same(model.ids.index(int(fids[2000])), "setTerms behind the column's end")
    # a setTerms that clears, one that replaces
    eng.setTerms(fids[50:60], [[]] * 10); model.set_terms(fids[50:60], [[]] * 10)
    eng.setTerms(fids[[70]], [[SESSION0, SESSION0 + 1, EVERYBODY, TAG0 + 2]]); model.set_terms(fids[[70]], [[SESSION0, SESSION0 + 1, EVERYBODY, TAG0 + 2]])
    same(model.ids.index(int(fids[50])), "clear and replace")
    # removing the tail and rows behind the column
    eng.removeBatch(fids[3500:4000]); model.remove_batch(fids[3500:4000])
    same(model.ids.index(int(fids[3499])) + 1, "removeBatch of the tail")
    # deserialize: every set is gone
    blob = eng.serialize()
    d0 = eng.termStats()["host_decided"]
    eng.deserialize(blob); model.drop_terms()
    same(None, "deserialize")
    assert eng.termStats()["host_decided"] == d0 + len(reqs) * len(queries)
    eng.setTerms(fids[:10], sets[:10]); model.set_terms(fids[:10], sets[:10])
    same(0, "terms again")
    eng.close()


def test_three_shards_on_one_device_equal_the_single_engine(wax):
    n, dims = 3000, 64
    one = Store(wax, "cosine", n, dims, seed=41, sessions=3)
    many = Store(wax, "cosine", n, dims, seed=41, sessions=3, devices=[0, 0, 0])
    assert many.eng.shardCount == 3 and all(many.eng.shardInfo(g)[2] > 0 for g in range(3))
    reqs = ([SESSION0], [SESSION0 + 2, TAG0 + 1], [EVERYBODY, TAG0 + 12])

    def both(sets, fids):
        for s in (one, many):
            s.sets, s.fids = sets, fids
        for qi, req in enumerate(reqs):
            for kw in ({}, {"timeRange": (10, 70)}, {"frameIds": fids[::3]}, {"minScore": 0.0}):
                a, b = one.check(req, 10, qi, **kw), many.check(req, 10, qi, **kw)
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32)), (req, kw)
        for f in fids[::97]:
            assert one.eng.getTerms(int(f)).tolist() == many.eng.getTerms(int(f)).tolist() == sorted(sets[fids.tolist().index(int(f))])

    both(one.sets, one.fids)
    assert many.eng.termStats()["device_masks"] >= 3 * len(reqs)
    # growth past every shard's block doubles the blocks: rows move between shards and take their sets with them
    r0 = many.eng.getTuning("rebalances")
    extra_rows, _ = corpus(6000, dims, 43)
    extra_ids = np.arange(6000, dtype=np.uint64) * 3 + 100_000
    extra_sets = term_sets(6000, 47, sessions=3)
    for s in (one, many):
        s.eng.addBatch(extra_ids, extra_rows)
        assert s.eng.setTerms(extra_ids[:4000], extra_sets[:4000]) == 4000
        s.eng.remove(int(one.fids[10]))
    assert many.eng.getTuning("rebalances") > r0
    keep = np.arange(n) != 10
    fids = np.concatenate([one.fids[keep], extra_ids])
    sets = [t for t, k in zip(one.sets, keep) if k] + extra_sets[:4000] + [()] * 2000
    both(sets, fids)
    one.eng.close()
    many.eng.close()
