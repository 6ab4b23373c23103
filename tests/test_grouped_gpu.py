"""The grouped search on the device (wax_amd/csrc/grouped.hip; wax_hip_search_grouped / _set_parents / _group_probe) against the
restatement of its contract in tests/grouped_ref.py. Every answer is array_equal to the model: roots, score bits, member ids, member
score bits, counts and padding.

Stores hold at most 10 000 rows, so that searchBatchHits with topK = rows yields every row's exact key for the model. The engine
route runs at 257, 4 097 and 9 999 rows with "grid_blocks" 1, 2 and 3, so that one workgroup walks many chunks; the probe sets
distances bit for bit on 20 000 rows."""
import ctypes

import numpy as np
import pytest

import grouped_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def wax():
    import wax_amd
    if not wax_amd.HIPVectorEngine.isAvailable():
        pytest.skip("no gfx950 device")
    return wax_amd


# ---- through the probe ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ref.PROBE_CASES, ids=lambda c: c.name)
def test_probe_equals_model(wax, case):
    exp = ref.probe_expected(case)
    n = len(exp.roots)
    if case.parents is None:
        slots, slot_root = None, case.frame_ids
    else:
        slots, slot_root = ref.slots_of(case.parents, case.frame_ids)
    bitmap = None if case.passing is None else ref.bitmap_of(case.passing)
    for grid in ref.GRIDS + (0,):                               # 0: the product's own grid
        roots, rkeys, mkeys, got = wax.groupProbe(case.dist, slots, slot_root, case.limit, case.per_group, bitmap=bitmap, grid=grid)
        assert got == n, grid
        assert np.array_equal(roots[:n], exp.roots) and (roots[n:] == ref.ID_PAD).all(), grid
        assert np.array_equal(rkeys[:n], exp.member_keys[:, 0]) and (rkeys[n:] == ref.KEY_PAD).all(), grid
        assert np.array_equal(mkeys[:n], exp.member_keys) and (mkeys[n:] == ref.KEY_PAD).all(), grid


# ---- through an engine ------------------------------------------------------------------------------------------------------

METRICS = {"cosine": 0, "dot": 1, "l2": 2}


def corpus(n, dims, seed):
    """Gaussian rows of which about a sixth repeat an earlier row bit for bit: equal distances across roots and within one."""
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((n, dims)).astype(np.float32)
    dup = np.nonzero(rng.random(n) < 0.17)[0]
    dup = dup[dup > 0]
    rows[dup] = rows[rng.integers(0, dup)]                       # chains of copies included: the source is read as it is by then
    return rows, rng.standard_normal(dims).astype(np.float32)


def engine(wax, metric, dims, fids, rows, devices=None):
    from wax_amd import VectorMetric
    eng = wax.HIPVectorEngine(metric=getattr(VectorMetric, metric), dimensions=dims, devices=devices)
    eng.addBatch(fids, rows)
    return eng


def row_keys(eng, q):
    """Every row's exact key (the bits wax_hip_search gives it), by row."""
    hits, _ = eng.searchBatchHits(q[None, :], eng.count)
    keys = hits[0, :, 0]
    keys = keys[keys != ref.KEY_PAD]
    assert len(keys) == eng.count
    by_row = np.empty(eng.count, dtype=np.int64)
    by_row[ref.key_rows(keys)] = keys
    finite = np.isfinite(ref.unorder_bits(ref.key_bits(by_row)))
    return np.where(finite, by_row, ref.KEY_PAD)


def check(eng, q, keys, parents, fids, passing, limit, per_group, metric="cosine", min_score=None, time_range=None, deny=0):
    exp = ref.grouped_model(keys, parents, fids, passing, limit, per_group)
    if min_score is not None:
        exp = ref.apply_cut(exp, min_score, metric)
    roots, scores, mids, mscores, counts = eng.searchGrouped(q, limit, per_group, timeRange=time_range, denyFlags=deny, minScore=min_score)
    what = (eng.count, limit, per_group)
    width = max(1, min(per_group, ref.MAX_MEMBERS))
    assert np.array_equal(roots, exp.roots), what
    assert np.array_equal(scores.view(np.int32), ref.score_of(exp.bits, metric).view(np.int32)), what
    assert np.array_equal(counts, exp.counts) and mids.shape == (len(exp.roots), width), what
    filled = exp.member_keys != ref.KEY_PAD
    exp_ids = np.where(filled, np.asarray(fids, dtype=np.uint64)[ref.key_rows(exp.member_keys) % len(fids)], ref.ID_PAD)
    exp_scores = np.where(filled, ref.score_of(ref.key_bits(exp.member_keys), metric), np.float32(0.0)).astype(np.float32)
    assert np.array_equal(mids, exp_ids), what
    assert np.array_equal(mscores.view(np.int32), exp_scores.view(np.int32)), what
    return roots, scores


PER_GROUPS = (1, 3, 8)


@pytest.mark.parametrize("n", (257, 4097, 9999))
def test_engine_route_equals_model(wax, n):
    dims = 384
    rows, q = corpus(n, dims, seed=n)
    stats = []
    for kind in ("none", "one", "scattered", "foreign"):
        parents, fids = ref.partition(kind, n, seed=n)
        eng = engine(wax, "cosine", dims, fids, rows)
        if parents is not None:
            assert eng.setParents(fids, parents) == n
        keys = row_keys(eng, q)
        n_groups = len(set(ref.roots_of(parents, fids).tolist()))
        for grid in (1, 2, 3):
            eng.setTuning("grid_blocks", grid)
            for limit in (1, 12, 1024):
                for per_group in PER_GROUPS:                     # 8 is more than most groups hold, and than every singleton
                    check(eng, q, keys, parents, fids, None, limit, per_group)
        if n_groups < 1024:                                      # a limit above the number of groups returns them all
            roots, _ = check(eng, q, keys, parents, fids, None, 1024, 2)
            assert len(roots) == n_groups
        if kind == "none":
            # frame ids ascend with the rows: the grouped answer is the ordinary search's, ids and score bits
            for k in (1, 10, 150):
                ids, scores = eng.searchArrays(q, k)
                roots, gscores, mids, _, counts = eng.searchGrouped(q, k)
                assert np.array_equal(roots, ids) and np.array_equal(gscores.view(np.int32), scores.view(np.int32))
                assert np.array_equal(mids[:, 0], ids) and (counts == 1).all()
        st = eng.groupStats()
        assert st["fused_scans"] == st["searches"] > 0 and st["column_scans"] == 0
        assert st["group_slots"] == (n if kind == "none" else n_groups)
        assert st["parent_rows_uploaded"] == (0 if kind == "none" else n)   # one upload, at the first search after setParents
        stats.append(st)
    assert stats[0]["member_rounds"] > 0


def test_predicates_and_cut(wax):
    n, dims = 4097, 384
    rows, q = corpus(n, dims, seed=11)
    parents, fids = ref.partition("scattered", n, seed=11)
    eng = engine(wax, "cosine", dims, fids, rows)
    eng.setParents(fids, parents)
    rng = np.random.default_rng(12)
    roots = ref.roots_of(parents, fids)
    # whole groups on one side of the time bound (the predicate empties them), the others split by a flag
    uniq = np.unique(roots)
    old = np.isin(roots, uniq[rng.random(len(uniq)) < 0.4])
    ts = np.where(old, 5, 50).astype(np.int64)
    flags = (rng.random(n) < 0.3).astype(np.uint32) * np.uint32(2)
    assert eng.setAttributes(fids, ts, flags) == n
    keys = row_keys(eng, q)
    eng.setTuning("grid_blocks", 2)
    for limit, per_group in ((12, 3), (1024, 8), (1, 1)):
        check(eng, q, keys, parents, fids, ~old, limit, per_group, time_range=(10, None))
        check(eng, q, keys, parents, fids, ~old & (flags == 0), limit, per_group, time_range=(10, None), deny=2)
        check(eng, q, keys, parents, fids, np.zeros(n, dtype=bool), limit, per_group, time_range=(60, None))   # nothing passes
    full = ref.grouped_model(keys, parents, fids, None, 1024, 8)
    g_scores = ref.score_of(full.bits)
    for cut in (float(g_scores[len(g_scores) // 2]), float(g_scores[5]), 2.0, -2.0):
        check(eng, q, keys, parents, fids, None, 1024, 8, min_score=cut)
        check(eng, q, keys, parents, fids, None, 12, 3, min_score=cut)


@pytest.mark.parametrize("metric,dims,n", [("cosine", 768, 1031), ("cosine", 20, 1031), ("dot", 384, 1031), ("l2", 384, 1031), ("l2", 20, 515)])
def test_other_dimensions_and_metrics(wax, metric, dims, n):
    rows, q = corpus(n, dims, seed=dims + n)
    parents, fids = ref.partition("scattered", n, seed=dims)
    eng = engine(wax, metric, dims, fids, rows)
    eng.setParents(fids, parents)
    keys = row_keys(eng, q)
    for grid in (1, 3):
        eng.setTuning("grid_blocks", grid)
        for limit, per_group in ((12, 3), (1024, 8)):
            check(eng, q, keys, parents, fids, None, limit, per_group, metric=metric)
    st = eng.groupStats()
    assert (st["column_scans"] == st["searches"] and st["fused_scans"] == 0) if dims == 20 else (st["fused_scans"] == st["searches"])
    if dims != 20:                                               # "force_general": the column route on a dimension the fused scan serves
        eng.setTuning("force_general", 1)
        check(eng, q, keys, parents, fids, None, 12, 3, metric=metric)
        assert eng.groupStats()["column_scans"] == 1


# ---- lifecycle --------------------------------------------------------------------------------------------------------------

class Model:
    """The store as the test knows it: rows in order, each (frame id, vector, parent)."""

    def __init__(self, dims, seed):
        self.dims, self.rng = dims, np.random.default_rng(seed)
        self.ids, self.vecs, self.parents = [], [], []

    def vectors(self, n):
        return self.rng.standard_normal((n, self.dims)).astype(np.float32)

    def add(self, ids, vecs):
        for i, v in zip(ids, vecs):
            if i in self.ids:
                self.vecs[self.ids.index(i)] = v                # an upsert keeps its row and its parent
            else:
                self.ids.append(i); self.vecs.append(v); self.parents.append(int(ref.NO_PARENT))   # an appended row is its own root

    def set_parents(self, ids, parents):
        for i, p in zip(ids, parents):
            if i in self.ids:
                self.parents[self.ids.index(i)] = int(p)

    def remove(self, ids):
        for i in ids:
            if i in self.ids:
                at = self.ids.index(i)
                del self.ids[at], self.vecs[at], self.parents[at]

    def drop_parents(self):
        self.parents = [int(ref.NO_PARENT)] * len(self.ids)


def test_lifecycle_follows_a_rebuilt_store(wax):
    dims = 64
    m = Model(dims, 21)
    eng = wax.HIPVectorEngine(dimensions=dims)
    q = m.rng.standard_normal(dims).astype(np.float32)
    NP = int(ref.NO_PARENT)

    def compare(step):
        fids = np.array(m.ids, dtype=np.uint64)
        assert eng.count == len(fids), step
        got_par, found = eng.getParents(fids)
        assert found.all() and np.array_equal(got_par, np.array(m.parents, dtype=np.uint64)), step
        fresh = wax.HIPVectorEngine(dimensions=dims)
        if len(fids):
            fresh.addBatch(fids, np.stack(m.vecs))
            if any(p != NP for p in m.parents):
                fresh.setParents(fids, np.array(m.parents, dtype=np.uint64))
        for limit, per_group in ((12, 3), (1024, 8), (3, 1)):
            a = eng.searchGrouped(q, limit, per_group)
            b = fresh.searchGrouped(q, limit, per_group)
            for x, y in zip(a, b):
                assert x.dtype == y.dtype and np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y), step
            if len(fids):
                keys = row_keys(fresh, q)
                check(eng, q, keys, np.array(m.parents, dtype=np.uint64), fids, None, limit, per_group)

    def uploaded():
        return eng.groupStats()["parent_rows_uploaded"]

    compare("empty")
    ids = list(range(1000, 1600))
    v = m.vectors(600); eng.addBatch(np.array(ids, dtype=np.uint64), v); m.add(ids, v)
    compare("add")
    assert uploaded() == 0                                       # no parent was ever set: nothing to upload
    par = [5_000_000 + (i % 37) if i % 5 else NP for i in ids]
    assert eng.setParents(np.array(ids + [42], dtype=np.uint64), np.array(par + [7], dtype=np.uint64)) == 600   # 42 is not held
    m.set_parents(ids, par)
    compare("setParents")
    assert uploaded() == 600
    compare("again")
    assert uploaded() == 600                                     # nothing changed: nothing uploaded
    # the last entry of a repeated id wins; a parent may be one of the store's own frames
    assert eng.setParents(np.array([1500, 1500, 1599], dtype=np.uint64), np.array([1, 1000, 1000], dtype=np.uint64)) == 3
    m.set_parents([1500, 1599], [1000, 1000])
    compare("repeated id")
    assert uploaded() == 600 + 100                               # from the lowest changed row (500) to the end
    up = [1003, 1250]
    v = m.vectors(2); eng.addBatch(np.array(up, dtype=np.uint64), v); m.add(up, v)
    compare("upsert")
    eng.remove(1010); m.remove([1010])
    compare("remove")
    assert uploaded() == 700 + (599 - 10)                        # rows behind the removed one shift their slot entries
    gone = list(range(1100, 1400, 3)) + [99999]
    assert eng.removeBatch(np.array(gone, dtype=np.uint64)) == 100
    m.remove(gone)
    compare("removeBatch")
    new = list(range(3000, 3300))
    v = m.vectors(300); eng.addBatch(np.array(new, dtype=np.uint64), v); m.add(new, v)
    before = uploaded()
    compare("append after set")
    assert uploaded() - before in (300, eng.count)               # the appended rows only — or the whole column where the store grew
    for i in (4000, 4001):                                       # staged single-frame appends are seen
        v = m.vectors(1); eng.add(i, v[0]); m.add([i], v)
    compare("add one")
    eng.setParents(np.array([4000, 4001, 3000], dtype=np.uint64), np.array([3000, 3000, NP], dtype=np.uint64))
    m.set_parents([4000, 4001, 3000], [3000, 3000, NP])
    compare("set on appended")
    eng.reserve(5000)
    compare("reserve")
    # removing most rows leaves most slots without a row: the numbering starts over
    most = m.ids[50:]
    eng.removeBatch(np.array(most, dtype=np.uint64)); m.remove(list(most))
    compare("mass removal")
    assert eng.groupStats()["group_slots"] <= 2 * eng.count + 16
    eng.deserialize(eng.serialize()); m.drop_parents()
    compare("deserialize")
    par, found = eng.getParents(np.array([m.ids[0], 123456], dtype=np.uint64))
    assert par.tolist() == [NP, NP] and found.tolist() == [True, False]


# ---- a handle ---------------------------------------------------------------------------------------------------------------

def test_handle_of_three_shards_equals_one_engine(wax):
    n, dims = 3001, 384
    rng = np.random.default_rng(31)
    rows = rng.standard_normal((n, dims)).astype(np.float32)
    q = rng.standard_normal(dims).astype(np.float32)
    fids = rng.permutation(n).astype(np.uint64)
    parents = np.uint64(9_000_000) + rng.integers(0, 300, size=n).astype(np.uint64)   # every group straddles the shards
    parents[rng.random(n) < 0.1] = ref.NO_PARENT
    # equal distances ACROSS roots (never inside one: which of two equal rows of different shards is "first" is the handle's layout)
    roots = ref.roots_of(parents, fids)
    for r in range(1, n, 9):
        if roots[r] != roots[r - 1]:
            rows[r] = rows[r - 1]
    one = engine(wax, "cosine", dims, fids, rows)
    one.setParents(fids, parents)
    sh = engine(wax, "cosine", dims, fids, rows, devices=[0, 0, 0])
    assert sh.setParents(fids, parents) == n
    got_par, found = sh.getParents(fids[:50])
    assert found.all() and np.array_equal(got_par, parents[:50])
    keys = row_keys(one, q)
    ts = rng.integers(0, 100, size=n).astype(np.int64)
    one.setAttributes(fids, ts, None); sh.setAttributes(fids, ts, None)
    for limit in (1, 12, 1024):
        for kw in ({}, {"timeRange": (30, None)}, {"minScore": 0.05}):
            a = one.searchGrouped(q, limit, 1, **kw)
            b = sh.searchGrouped(q, limit, 1, **kw)
            for x, y in zip(a, b):
                assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y), (limit, kw)
        check(sh, q, keys, parents, fids, None, limit, 1)
    from wax_amd.errors import WaxError
    with pytest.raises(WaxError) as ei:
        sh.searchGrouped(q, 12, 3)
    assert "per_group" in str(ei.value)
    st = sh.groupStats()
    assert st["searches"] > 0 and st["parent_rows_uploaded"] == n


# ---- refusals ---------------------------------------------------------------------------------------------------------------

def test_refusals_leave_outputs_untouched(wax):
    from wax_amd import _abi
    lib = _abi.lib()
    dims = 64
    eng = wax.HIPVectorEngine(dimensions=dims)
    rng = np.random.default_rng(41)
    eng.addBatch(np.arange(100, dtype=np.uint64), rng.standard_normal((100, dims)).astype(np.float32))
    q = rng.standard_normal(dims).astype(np.float32)
    f32p, u64p, u32p = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)

    def call(limit, per_group, use_q=True, n_dims=dims, roots=True, scores=True, mids=True, mscores=True, count=True, handle=True):
        out = {"roots": np.full(2048, 7, dtype=np.uint64), "scores": np.full(2048, 7, dtype=np.float32),
               "mids": np.full(2048 * 8, 7, dtype=np.uint64), "mscores": np.full(2048 * 8, 7, dtype=np.float32),
               "counts": np.full(2048, 7, dtype=np.uint32)}
        got = ctypes.c_uint32(77)
        rc = lib.wax_hip_search_grouped(eng._h if handle else None, q.ctypes.data_as(f32p) if use_q else None, n_dims, limit, per_group, 0, 0.0, None,
                                        out["roots"].ctypes.data_as(u64p) if roots else None, out["scores"].ctypes.data_as(f32p) if scores else None,
                                        out["mids"].ctypes.data_as(u64p) if mids else None, out["mscores"].ctypes.data_as(f32p) if mscores else None,
                                        out["counts"].ctypes.data_as(u32p), ctypes.byref(got) if count else None)
        return rc, got.value, out

    def untouched(out):
        return all((a == 7).all() for a in out.values())

    for kw in (dict(limit=1025, per_group=1), dict(limit=12, per_group=9), dict(limit=12, per_group=1, use_q=False),
               dict(limit=12, per_group=1, roots=False), dict(limit=12, per_group=1, scores=False), dict(limit=12, per_group=1, count=False),
               dict(limit=12, per_group=1, handle=False), dict(limit=12, per_group=2, mids=False), dict(limit=12, per_group=2, mscores=False)):
        rc, got, out = call(**kw)
        assert rc == _abi.ERR_INVALID_ARGUMENT and got == 77 and untouched(out), kw
    rc, got, out = call(limit=12, per_group=1, n_dims=65)
    assert rc == _abi.ERR_DIM_MISMATCH and got == 77 and untouched(out)
    assert _abi.last_error() == "vector dimension mismatch: expected 64, got 65"
    before = eng.groupStats()["searches"]
    for limit in (0, -5):                                        # count 0, no device touched
        rc, got, out = call(limit=limit, per_group=1)
        assert rc == _abi.OK and got == 0 and untouched(out)
    assert eng.groupStats()["searches"] == before
    rc, got, out = call(limit=3, per_group=0)                    # per_group < 1 is read as 1
    assert rc == _abi.OK and got == 3 and (out["counts"][:3] == 1).all() and (out["mids"][3:] == 7).all()
    rc, got, out = call(limit=3, per_group=2, mids=False, mscores=False)   # no members wanted
    assert rc == _abi.OK and got == 3 and (out["mids"] == 7).all()
    empty = wax.HIPVectorEngine(dimensions=dims)
    r = empty.searchGrouped(q, 12, 3)
    assert all(len(x) == 0 for x in r)
    # a thread that holds tickets may search, and is refused as a writer
    t = eng.submit(q, 5)
    assert len(eng.searchGrouped(q, 5)[0]) == 5
    from wax_amd.errors import WaxError
    with pytest.raises(WaxError):
        eng.setParents([1], [2])
    eng.collect(t, 5)
    assert eng.setParents([1], [2]) == 1
