"""The model behind tests/test_store_sequence_cpu.py and tests/test_store_sequence_gpu.py: one seeded stream of mutations per store,
the store it must leave (numpy only, no engine code), what every derived structure's counter must move by, and the float64 margins of
both mirror certificates.

The engine keeps six structures derived from the f32 store (bf16 mirror, 8-bit code mirror, id -> row table, attribute columns, the
bitmap entries of predicate tickets, the staging area of single adds). Each follows mutations by its own incremental protocol; a
search route that reads one of them gives a wrong answer, with a passing certificate, whenever the structure missed a mutation. The
GPU test replays a Sequence on an engine and, after every step, holds every route to a store rebuilt from this model.

Model      ordered frame ids, rows, ts, flags with the reference's semantics as helpers.OracleEngine has them: upsert by id (first
           row that holds the id), order-preserving remove of that first row, attributes (0, 0) for new rows and after deserialize.
Protocol   the host-side state machines of batch_host.inc / api_store.inc / codec.inc, restated rule by rule (each method names the
           engine function it restates), so the deltas of "mirror_rows_converted", "idhash_rows_inserted", "mirror8_conversions" and
           "mirror8_rows_converted" over one step (its mutations, then every reader) are predicted, and so the states a step enters are
           tagged with the coverage class they belong to.
Sequence   about 40 steps. A step is one to three mutations with no reader between them (the states the issue lists — an upsert of
           a row the mirror has not converted yet, a removal that renumbers listed dirty rows, growth with rows pending — only exist
           between two readers), then every reader. Every step is planted: an append or upsert puts in a row at cosine
           0.9 - 0.02 j to one of the 4 checked queries (scaled 0.8 .. 1.6 under dot), a removal takes a current top hit, an attribute
           step moves a current top hit across a checked predicate.

The rows of a sequence live in one pool (a row never changes; an upsert points the frame at another pool row), so the per-row terms of
both certificates are computed once per pool row."""
import functools

import numpy as np

import mirror8_planes_ref as P8
import mirror8_ref as R8
import oracle
import predicate_mirror_ref as PM

COS, DOT, L2 = 0, 1, 2
KS = (1, 10)
N_QUERIES = 4                    # checked queries per store
N_BATCH = 32                     # queries of the searchBatch reader (the 4 checked ones first)
K_MAX_DIRTY = 4096               # kMirrorMaxDirty (engine_types.inc)
INITIAL_RESERVE = 64             # WAX_HIP_INITIAL_RESERVE
COMPACT_WINDOW = 37              # "compact_window_rows" of the engine under test
TILE = 16                        # rows per tile of the code mirror
KP = 64                          # candidates either mirror re-scores
PLANT_LEVELS = 24
# the checked predicates, as keyword arguments of searchFiltered / submitFiltered
PRED_A = {"denyFlags": 1}                    # flag bit 0 ("deleted")
PRED_B = {"timeRange": (500, None)}          # new rows (ts 0) fail it until an attribute step moves them
PREDICATES = {"A": PRED_A, "B": PRED_B}
ABSENT_ID = 999_999_999_999

# name -> metric, rows, dims, seed, mirror-capable
CONFIGS = {
    "cos384": dict(metric=COS, n=5003, dims=384, seed=2801, mirror=True),
    "dot768": dict(metric=DOT, n=2101, dims=768, seed=2802, mirror=True),
    "l2_100": dict(metric=L2, n=700, dims=100, seed=2803, mirror=False),
}

# the coverage classes every mirror-capable sequence must enter (tags of Protocol and the generator)
MIRROR_CLASSES = (
    "upsert_converted", "upsert_above_fill", "upserts_4096_listed", "upserts_4097_stale",
    "remove_below_fill", "remove_dirty_below", "remove_dirty_above", "remove_dirty_at", "remove_above_fill",
    "remove_batch_straddle", "remove_batch_dirty_removed", "remove_batch_dirty_surviving",
    "compact_bounce", "compact_direct", "compact_several_windows", "compact_mirror_ends_inside_window", "compact_mirror_ends_below_window",
    "growth_dirty_pending", "growth_unconverted_pending", "append_in_tile", "dup_blob", "dup_remove_first_row", "dup_upsert_second_row",
    "remove_batch_loop_path",
)
OP_KINDS = ("addBatch", "add", "remove", "removeBatch", "setAttributes", "reserve", "roundtrip", "deserialize_blob")
L2_CLASSES = ("idhash_realloc", "growth", "remove_batch_plain", "dup_blob")


def passing(ts, fl, timeRange=None, denyFlags=0):
    """The numpy model of the row predicate (TimeRange.contains: after inclusive, before exclusive; any denied flag bit drops the row)."""
    m = (np.asarray(fl, dtype=np.uint32) & np.uint32(denyFlags)) == 0
    if timeRange is not None:
        after, before = timeRange
        if after is not None:
            m &= np.asarray(ts, dtype=np.int64) >= after
        if before is not None:
            m &= np.asarray(ts, dtype=np.int64) < before
    return m


# ---------------------------------------------------------------------------------------------------------------------------------
# the pool of rows

class Pool:
    """Every row a sequence ever stores, and its float64 distance to the checked queries (the model's ranking)."""

    def __init__(self, metric, dims, queries):
        self.metric, self.dims, self.queries = metric, dims, queries
        self.blocks, self.dist, self.n = [], [], 0
        self._rows = None

    def add(self, vecs):
        vecs = np.ascontiguousarray(vecs, dtype=np.float32).reshape(-1, self.dims)
        self.blocks.append(vecs)
        self.dist.append(exact_distances(self.metric, vecs, self.queries))
        self._rows = None
        first = self.n
        self.n += len(vecs)
        return np.arange(first, self.n, dtype=np.int64)

    @property
    def rows(self):
        if self._rows is None:
            self._rows = np.concatenate(self.blocks) if self.blocks else np.zeros((0, self.dims), dtype=np.float32)
            self.blocks = [self._rows]
            self._dist = np.concatenate(self.dist)
            self.dist = [self._dist]
        return self._rows

    @property
    def exact(self):
        self.rows
        return self._dist


def exact_distances(metric, rows, queries):
    """float64 distances [rows, queries] under the engine's three metrics (l2: squared, which ranks as the distance does)."""
    r, q = rows.astype(np.float64), queries.astype(np.float64)
    if metric == L2:
        return ((r[:, None, :] - q[None, :, :]) ** 2).sum(axis=2)
    return np.stack([R8.exact_distances(rows, qq, metric) for qq in queries], axis=1)


# ---------------------------------------------------------------------------------------------------------------------------------
# the store

class Model:
    """Ordered frame ids, pool rows, ts, flags. A frame id may sit in two rows only after deserialize_blob; every call by id then
    means the FIRST row that holds it (firstIndex(of:))."""

    def __init__(self):
        self.ids, self.rows, self.ts, self.fl = [], [], [], []

    @property
    def count(self):
        return len(self.ids)

    def find(self, fid):
        try:
            return self.ids.index(fid)
        except ValueError:
            return -1

    def upsert(self, fid, prow):
        i = self.find(fid)
        if i >= 0:
            self.rows[i] = prow
            return i, False
        self.ids.append(fid); self.rows.append(prow); self.ts.append(0); self.fl.append(0)
        return len(self.ids) - 1, True

    def remove(self, fid):
        i = self.find(fid)
        if i >= 0:
            for col in (self.ids, self.rows, self.ts, self.fl):
                del col[i]
        return i

    def set_attributes(self, ids, ts, fl):
        for j, fid in enumerate(ids):
            i = self.find(fid)
            if i < 0:
                continue
            if ts is not None:
                self.ts[i] = int(ts[j])
            if fl is not None:
                self.fl[i] = int(fl[j])

    def replace(self, ids, rows):
        self.ids, self.rows = [int(i) for i in ids], [int(r) for r in rows]
        self.ts, self.fl = [0] * len(self.ids), [0] * len(self.ids)

    def has_repeated_ids(self):
        return len(set(self.ids)) != len(self.ids)


class Snapshot:
    """The store after a step, as arrays."""

    def __init__(self, model):
        self.ids = np.array(model.ids, dtype=np.uint64)
        self.rows = np.array(model.rows, dtype=np.int64)
        self.ts = np.array(model.ts, dtype=np.int64)
        self.fl = np.array(model.fl, dtype=np.uint32)
        self.repeated = model.has_repeated_ids()

    @property
    def count(self):
        return len(self.ids)

    def mask(self, pred):
        """pred: None (unfiltered), "A" or "B"."""
        if pred is None:
            return np.ones(self.count, dtype=bool)
        return passing(self.ts, self.fl, **PREDICATES[pred])


# ---------------------------------------------------------------------------------------------------------------------------------
# the protocols

class Protocol:
    """The host-side state of the derived structures, moved by the same mutations as the engine's, restated from the engine's source.
    `tags` collects the coverage classes entered since it was last cleared."""

    def __init__(self, mirror_capable):
        self.mirror_capable = mirror_capable
        self.capacity, self.count, self.pend = INITIAL_RESERVE, 0, 0
        # bf16 mirror (BatchMirror: rows / dirty / stale, mirror_cap)
        self.m_init, self.m_cap, self.m_rows, self.m_dirty, self.m_stale = False, 0, 0, [], False
        # id -> row table (IdHash)
        self.h_valid, self.h_stale, self.h_rows, self.h_slots = False, False, 0, 0
        # 8-bit code mirror
        self.c_exists, self.c_cap, self.c_stale, self.c_valid, self.c_rows = False, 0, False, False, 0
        self.tags = set()

    # -- store_internal.inc: reserve_rows / resize_store
    def _reserve_rows(self, required):
        if required <= self.capacity:
            return
        nxt = self.capacity
        while required > nxt:
            nxt *= 2
        self.pend = 0                                     # resize_store flushes the staged rows
        self.capacity = nxt
        self.tags.add("growth")

    # -- batch_host.inc: c8_note_append / c8_note_stale
    def _c8_append(self):
        self.c_valid = False

    def _c8_stale(self):
        self.c_valid, self.c_stale = False, True

    # -- batch_host.inc: mirror_note_upsert
    def _upsert(self, row):
        self._c8_stale()
        if self.m_stale or row >= self.m_rows:
            if self.m_init and not self.m_stale:
                self.tags.add("upsert_above_fill")
            return
        if len(self.m_dirty) >= K_MAX_DIRTY:
            self.m_stale, self.m_dirty = True, []
            self.tags.add("upserts_4097_stale")
            return
        self.m_dirty.append(row)
        self.tags.add("upsert_converted")

    # -- api_store.inc: wax_hip_add_batch (n == 1 is add(frameId:vector:): the staging area)
    def add_batch(self, rows_hit):
        """rows_hit: per entry, the store row it overwrites or -1 for an append (the model decides; sequential upsert semantics)."""
        n = len(rows_hit)
        if n == 0:
            return
        if self.pend:
            self.tags.add("staged_pending:" + ("add" if n == 1 else "addBatch"))
        self.h_valid = False                              # mirror_note_append
        self._c8_append()
        if n == 1:
            if rows_hit[0] >= 0:
                self._upsert(rows_hit[0])
                return
            self._reserve_rows(self.count + 1)
            self.pend += 1
            self.count += 1
            return
        self.pend = 0                                     # flush_pending
        self._reserve_rows(self.count + n)                # upper bound: every id new
        for r in rows_hit:
            if r >= 0:
                self._upsert(r)
            else:
                self.count += 1
        if len(self.m_dirty) == K_MAX_DIRTY and not self.m_stale:
            self.tags.add("upserts_4096_listed")

    # -- api_store.inc: wax_hip_remove + batch_host.inc: mirror_note_remove
    def remove(self, idx, loop=False):
        if idx < 0:
            if self.pend:
                self.tags.add("staged_pending:remove_absent")
            return                                        # :426 before anything is touched
        if self.pend and not loop:
            self.tags.add("staged_pending:remove")
        self.pend = 0
        self.h_valid, self.h_stale, self.h_rows = False, True, 0
        self._c8_stale()
        if not (self.m_stale or self.m_cap == 0 or idx >= self.m_rows):
            self.tags.add("remove_below_fill")
            if any(r < idx for r in self.m_dirty):
                self.tags.add("remove_dirty_below")
            if any(r > idx for r in self.m_dirty):
                self.tags.add("remove_dirty_above")
            if any(r == idx for r in self.m_dirty):
                self.tags.add("remove_dirty_at")
            self.m_rows -= 1
            self.m_dirty = [r - 1 if r > idx else r for r in self.m_dirty if r != idx]
        elif self.m_cap and not self.m_stale:
            self.tags.add("remove_above_fill")
        self.count -= 1

    # -- api_store.inc: wax_hip_remove_batch + batch_host.inc: compact_removed_rows, mirror_note_remove_batch
    def remove_batch(self, rem):
        """rem: the store rows that leave, ascending and distinct (a store without repeated ids)."""
        if self.pend:
            self.tags.add("staged_pending:removeBatch")
        self.pend = 0
        if not rem:
            return
        m = len(rem)
        self.tags.add("remove_batch_plain")
        follow = not self.m_stale and self.m_cap != 0 and rem[0] < self.m_rows
        if rem[0] + m < self.count:
            self._compact_windows(rem, self.m_rows if follow else 0)
        self.h_valid, self.h_stale, self.h_rows = False, True, 0
        self._c8_stale()
        if not (self.m_stale or self.m_cap == 0 or rem[0] >= self.m_rows):
            gone = set(rem)
            if rem[-1] >= self.m_rows:
                self.tags.add("remove_batch_straddle")
            if any(r in gone for r in self.m_dirty):
                self.tags.add("remove_batch_dirty_removed")
            if any(r not in gone and r > rem[0] for r in self.m_dirty):
                self.tags.add("remove_batch_dirty_surviving")
            rank = lambda r: int(np.searchsorted(rem, r, side="left"))
            self.m_rows -= rank(self.m_rows)
            self.m_dirty = [r - rank(r) for r in self.m_dirty if r not in gone]
        self.count -= m

    def _compact_windows(self, rem, mirror_rows):
        """The window loop of compact_removed_rows, for its tags only: which forms ran, and where the mirror's fill fell."""
        m, count, window = len(rem), self.count, COMPACT_WINDOW
        w0, p, windows = rem[0], 0, 0
        while True:
            while p < m and rem[p] == w0:
                p += 1; w0 += 1
            if w0 >= count:
                break
            direct = p >= window
            w1 = min(count, w0 + (p if direct else window))
            self.tags.add("compact_direct" if direct else "compact_bounce")
            if mirror_rows:
                if mirror_rows <= w0:
                    self.tags.add("compact_mirror_ends_below_window")       # the `r.limit <= w0` arm
                elif mirror_rows < w1:
                    self.tags.add("compact_mirror_ends_inside_window")      # the `rank_limit` arm
            p = int(np.searchsorted(rem, w1, side="left"))
            w0 = w1
            windows += 1
        if windows > 1:
            self.tags.add("compact_several_windows")

    def set_attributes(self):
        if self.pend:
            self.tags.add("staged_pending:setAttributes")

    def reserve(self, rows):
        if self.pend:
            self.tags.add("staged_pending:reserve")
        self._reserve_rows(rows)

    # -- codec.inc: wax_hip_deserialize (mirror_note_replaced; capacity only grows, to the segment's rows exactly)
    def deserialize(self, n, kind):
        if self.pend:
            self.tags.add("staged_pending:" + kind)
        self.m_stale, self.m_dirty, self.m_rows = True, [], 0
        self.h_valid, self.h_stale, self.h_rows = False, True, 0
        self._c8_stale()
        self.pend = 0
        if n > self.capacity:
            self.capacity = n
            self.tags.add("growth")
        self.count = n

    def flush(self):
        """serialize() is a reader of the staging area."""
        self.pend = 0

    # -- the readers: ensure_mirror, ensure_idhash, mirror8_take + ensure_mirror8 (at least three eligible queries run per step)
    def read(self):
        self.pend = 0
        out = {"mirror_rows_converted": 0, "idhash_rows_inserted": 0, "mirror8_conversions": 0, "mirror8_rows_converted": 0}
        if self.mirror_capable and self.count:
            if not self.m_init:
                self.m_init, self.m_stale = True, True
            if self.m_cap < self.capacity:
                if not self.m_stale and self.m_rows > 0 and self.m_cap:
                    if self.m_dirty:
                        self.tags.add("growth_dirty_pending")
                    if self.m_rows < self.count:
                        self.tags.add("growth_unconverted_pending")
                else:
                    self.m_stale = True
                self.m_cap = self.capacity
            if self.m_stale:
                self.m_rows, self.m_dirty, self.m_stale = 0, [], False
            out["mirror_rows_converted"] = max(self.count - self.m_rows, 0) + len(set(self.m_dirty))
            self.m_rows, self.m_dirty = self.count, []
        if not self.h_valid and self.count:
            want = 1024
            while want < 2 * self.count:
                want *= 2
            if self.h_slots < want:
                if self.h_slots:
                    self.tags.add("idhash_realloc")
                self.h_slots, self.h_stale = 2 * want, True
            if self.h_stale:
                self.h_rows, self.h_stale = 0, False
            out["idhash_rows_inserted"] = self.count - self.h_rows
            self.h_rows, self.h_valid = self.count, True
        if self.mirror_capable and self.count and not (self.c_valid and self.c_cap >= self.capacity):
            if self.c_cap >= self.capacity and self.c_exists and not self.c_stale:
                # only appended rows are missing: converted at once by the first eligible query
                if self.c_rows < self.count:
                    if self.c_rows % TILE:
                        self.tags.add("append_in_tile")
                    out["mirror8_conversions"], out["mirror8_rows_converted"] = 1, self.count - self.c_rows
            else:
                # stale, missing or too small: one whole conversion, by the third eligible query
                out["mirror8_conversions"], out["mirror8_rows_converted"] = 1, self.count
            self.c_exists, self.c_cap, self.c_stale, self.c_valid, self.c_rows = True, self.capacity, False, True, self.count
        return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the sequence

class Step:
    def __init__(self, name, ops):
        self.name, self.ops = name, ops
        self.tags, self.after, self.counters = set(), None, None


class Sequence:
    """What generate() returns: the pool, the queries, the steps (ops, tags, the store after them, the predicted counter deltas)."""

    def __init__(self, name, cfg, pool, queries, batch_queries, steps):
        self.name, self.cfg, self.pool, self.queries, self.batch_queries, self.steps = name, cfg, pool, queries, batch_queries, steps
        self.metric, self.dims, self.mirror = cfg["metric"], cfg["dims"], cfg["mirror"]

    def tags(self):
        out = set()
        for s in self.steps:
            out |= s.tags
        return out

    def matrix(self, snap):
        return self.pool.rows[snap.rows]

    def top(self, snap, qi, pred, k=10):
        """The float64 top-k of query qi among the rows that pass `pred`: (frame ids, pool rows), best first, row order breaks ties."""
        rows = np.flatnonzero(snap.mask(pred))
        d = self.pool.exact[snap.rows[rows], qi]
        order = np.lexsort((rows, d))[:k]
        return snap.ids[rows[order]], snap.rows[rows[order]]


class _Gen:
    def __init__(self, name):
        cfg = CONFIGS[name]
        self.name, self.cfg = name, cfg
        self.metric, self.dims, self.n0 = cfg["metric"], cfg["dims"], cfg["n"]
        self.rng = np.random.default_rng(cfg["seed"])
        allq = oracle.gaussian_unit_queries(N_BATCH, self.dims, seed=cfg["seed"])
        self.queries, self.batch_queries = allq[:N_QUERIES], allq
        self.pool = Pool(self.metric, self.dims, self.queries)
        self.model, self.proto = Model(), Protocol(cfg["mirror"])
        self.steps, self.planted, self.next_id = [], 0, 10 ** 6

    # -- rows
    def rand_rows(self, n):
        x = self.rng.standard_normal((n, self.dims))
        x /= np.linalg.norm(x, axis=1)[:, None]
        if self.metric == DOT:
            x *= self.rng.uniform(0.5, 2.0, size=(n, 1))
        return self.pool.add(x.astype(np.float32))

    def plant(self, qi):
        """One row at cosine 0.9 - 0.02 j to query qi (a small step further down after every 24), scaled 0.8 .. 1.6 under dot."""
        j = self.planted
        self.planted += 1
        c = 0.9 - 0.02 * (j % PLANT_LEVELS) - 0.0007 * (j // PLANT_LEVELS)
        q = self.queries[qi].astype(np.float64)
        q /= np.linalg.norm(q)
        u = self.rng.standard_normal(self.dims)
        u -= (u @ q) * q
        u /= np.linalg.norm(u)
        v = c * q + np.sqrt(1.0 - c * c) * u
        if self.metric == DOT:
            v *= 0.8 + 0.8 * ((j * 7) % 11) / 10.0
        return int(self.pool.add(v.astype(np.float32))[0])

    def new_ids(self, n):
        out = list(range(self.next_id, self.next_id + n))
        self.next_id += n
        return out

    # -- the model's view
    def snap(self):
        return Snapshot(self.model)

    def pool_top_ids(self, snap, qi, k):
        d = self.pool.exact[snap.rows, qi]
        return snap.ids[np.lexsort((np.arange(snap.count), d))[:k]]

    def top_hit(self, qi, pred=None, rank=0):
        s = self.snap()
        rows = np.flatnonzero(s.mask(pred))
        d = self.pool.exact[s.rows[rows], qi]
        return int(s.ids[rows[np.lexsort((rows, d))[rank]]])

    # -- one step: apply every op to the model and the protocol, then read
    def step(self, name, ops, then=None):
        """`then`: a callable that returns further ops once `ops` have been applied (ops that name rows the first ones made)."""
        st = Step(name, list(ops))
        self.proto.tags = set()
        for op in st.ops:
            self.apply(op)
        if then is not None:
            more = then()
            for op in more:
                self.apply(op)
            st.ops += more
        st.counters = self.proto.read()
        st.tags = set(self.proto.tags) | getattr(self, "_extra_tags", set())
        self._extra_tags = set()
        st.after = self.snap()
        self.steps.append(st)
        return st

    def tag(self, *names):
        self._extra_tags = getattr(self, "_extra_tags", set()) | set(names)

    def apply(self, op):
        kind, m, p = op[0], self.model, self.proto
        if kind in ("addBatch", "add"):
            ids, rows = (op[1], op[2]) if kind == "addBatch" else ([op[1]], [op[2]])
            hit = []
            for fid, prow in zip(ids, rows):
                i, new = m.upsert(int(fid), int(prow))
                hit.append(-1 if new else i)
            p.add_batch(hit)
        elif kind == "remove":
            repeated = m.has_repeated_ids()
            i = m.remove(int(op[1]))
            if repeated and i >= 0:
                self.tag("dup_remove_first_row")
            p.remove(i)
        elif kind == "removeBatch":
            if m.has_repeated_ids():                      # the per-id loop of wax_hip_remove_batch
                self.tag("remove_batch_loop_path")
                if p.pend:
                    p.tags.add("staged_pending:removeBatch")
                p.pend = 0
                for fid in op[1]:
                    i = m.remove(int(fid))
                    if i >= 0:
                        self.tag("dup_remove_first_row")
                    p.remove(i, loop=True)
            else:
                rem = sorted({m.find(int(fid)) for fid in op[1]} - {-1})
                p.remove_batch(rem)
                for fid in op[1]:
                    m.remove(int(fid))
        elif kind == "setAttributes":
            p.set_attributes()
            m.set_attributes(op[1], op[2], op[3])
        elif kind == "reserve":
            p.reserve(int(op[1]))
        elif kind == "roundtrip":
            if p.pend:
                p.tags.add("staged_pending:roundtrip")
            p.flush()
            p.deserialize(m.count, "roundtrip")
            m.replace(m.ids, m.rows)
        elif kind == "deserialize_blob":
            p.deserialize(len(op[1]), "deserialize_blob")
            m.replace(op[1], op[2])
            if m.has_repeated_ids():
                self.tag("dup_blob")
        else:
            raise AssertionError(kind)

    # -- op builders
    def id_at(self, row):
        return self.model.ids[row]

    def attrs_for(self, ids):
        """Fresh attribute values for the listed frames: ts 1000 + its place in the list, flag bit 0 on about three in ten."""
        ts = 1000 + np.arange(len(ids), dtype=np.int64)
        fl = (self.rng.random(len(ids)) < 0.3).astype(np.uint32)
        return ("setAttributes", [int(i) for i in ids], ts, fl)


def _build(name):
    g = _Gen(name)
    m, rng, mirror = g.model, g.rng, g.cfg["mirror"]
    base_ids = [int(i) * 3 + 7 for i in range(g.n0)]
    g.step("build", [("addBatch", base_ids, list(g.rand_rows(g.n0))), g.attrs_for(base_ids)])

    def some_rows(n, lo=0, hi=None):
        return sorted(int(r) for r in rng.choice(np.arange(lo, m.count if hi is None else hi), n, replace=False))

    # 1 an upsert of converted rows
    r = some_rows(3)
    g.step("upsert of converted rows", [("addBatch", [g.id_at(x) for x in r], [g.plant(0), g.plant(1), g.plant(2)])])
    # 2 an append that begins inside a 16-row tile of the (by now valid) code mirror
    g.step("append inside a tile", [("addBatch", g.new_ids(5), [g.plant(3)] + list(g.rand_rows(2)) + [g.plant(0)] + list(g.rand_rows(1)))])
    # 3 an id repeated inside one batch: its second entry upserts a row the mirror has not converted
    a, b = g.new_ids(2)
    g.step("append and upsert of the appended row", [("addBatch", [a, b, a], list(g.rand_rows(2)) + [g.plant(1)])])
    # 4 staged single adds, one of them an upsert of a converted row while rows are staged
    g.step("staged adds", [("add", g.new_ids(1)[0], g.plant(2)), ("add", g.new_ids(1)[0], int(g.rand_rows(1)[0])),
                           ("add", g.id_at(some_rows(1)[0]), g.plant(3))])
    # 5 a removal of a top hit with a staged row pending, an absent id first
    g.step("staged add, remove", [("add", g.new_ids(1)[0], int(g.rand_rows(1)[0])), ("remove", ABSENT_ID), ("remove", g.top_hit(0))])
    # 6 a removal below the fill with listed dirty rows below it, at it and above it
    r = some_rows(3, 50, g.n0 - 50)
    g.step("remove among dirty rows", [("addBatch", [g.id_at(x) for x in r], [g.plant(0), g.plant(1), g.plant(2)]), ("remove", g.id_at(r[1]))])
    # 7 a removal at or above the fill
    ids = g.new_ids(3)
    g.step("remove above the fill", [("addBatch", ids, [g.plant(3), g.plant(0), int(g.rand_rows(1)[0])]), ("remove", ids[0])])
    # 8 an attribute step: a top hit of predicate A gets the denied flag
    g.step("flag flip", [("setAttributes", [g.top_hit(1, "A")], None, np.array([1], dtype=np.uint32))])
    # 9 removeBatch straddling the fill, several windows of 37 rows in both forms, dirty rows among the removed and the surviving
    fill = m.count
    s0 = fill - 300
    dirty = [s0 - 20, s0 + 120, s0 + 200, fill - 30]
    ops = [("addBatch", [g.id_at(x) for x in dirty], [g.plant(1), int(g.rand_rows(1)[0]), g.plant(2), int(g.rand_rows(1)[0])]),
           ("add", g.new_ids(1)[0], int(g.rand_rows(1)[0]))]
    new = g.new_ids(60)
    ops.append(("addBatch", new, list(g.rand_rows(59)) + [g.plant(3)]))

    def gone():
        rows = [s0 + 3, s0 + 10, s0 + 11] + list(range(s0 + 50, s0 + 95)) + [s0 + 120] + list(range(fill - 5, fill + 10)) + [fill + 30]
        return [("removeBatch", [g.id_at(x) for x in rows] + [g.top_hit(2), ABSENT_ID, g.id_at(s0 + 10)])]

    g.step("removeBatch across the fill", ops, then=gone)
    # 10 an attribute step: an unfiltered top hit with ts 0 moves into predicate B
    s = g.snap()
    cand = [int(i) for i in g.pool_top_ids(s, 0, 10) if s.ts[list(s.ids).index(i)] < 500]
    g.step("ts move", [("setAttributes", [cand[0]], np.array([2000], dtype=np.int64), None)])
    # 11 growth with dirty and unconverted rows pending
    r = some_rows(2)
    g.step("reserve with rows pending", [("addBatch", [g.id_at(x) for x in r], [g.plant(1), int(g.rand_rows(1)[0])]),
                                         ("addBatch", g.new_ids(3), [g.plant(2)] + list(g.rand_rows(2))),
                                         ("reserve", g.proto.capacity * 2)])
    # 12 the engine's own blob, with a staged row in front of it; 13 attributes come back
    g.step("serialize, deserialize", [("add", g.new_ids(1)[0], g.plant(3)), ("roundtrip",)])
    g.step("attributes again", [g.attrs_for(m.ids[::-1][: (m.count * 4) // 5])])
    if mirror:
        # 14 / 16 exactly 4 096 listed upserts in one addBatch (the list holds them), then 4 097 (it overflows: stale)
        for n_up, label in ((K_MAX_DIRTY, "4096 upserts"), (K_MAX_DIRTY + 1, "4097 upserts")):
            base = some_rows(min(n_up, m.count - 5))       # a store below 4 096 rows lists its rows more than once
            rows = (base * (n_up // len(base) + 1))[:n_up]
            vec = list(g.rand_rows(n_up))
            vec[-1] = g.plant(0)
            vec[7] = g.plant(1)
            g.step(label, [("addBatch", [g.id_at(x) for x in rows], vec)])
            if n_up == K_MAX_DIRTY:
                g.step("remove a top hit", [("remove", g.top_hit(0))])
    else:
        # the id table crosses its reallocation point (2 048 rows: the load factor passes 0.5 at 4 096 slots)
        ids = g.new_ids(1500)
        vec = list(g.rand_rows(1500))
        vec[3], vec[900] = g.plant(0), g.plant(1)
        g.step("growth past 2048 rows", [("addBatch", ids, vec)])
        g.step("remove a top hit", [("remove", g.top_hit(0))])
    # a segment of another writer in which two rows share a frame id: every call by id means the lower row
    s = g.snap()
    ids, rows = list(s.ids), list(s.rows)
    lower, upper = 10, 11
    ids[upper] = ids[lower]
    rows[lower] = g.plant(2)
    shared = int(ids[lower])
    g.step("two rows, one id", [("add", g.new_ids(1)[0], int(g.rand_rows(1)[0])), ("deserialize_blob", ids, rows)])   # (the staged row is dropped)
    g.step("removeBatch of the shared id", [("add", g.new_ids(1)[0], g.plant(3)), ("removeBatch", [shared, ABSENT_ID])])
    g.tag("dup_upsert_second_row")
    g.step("upsert of the shared id", [("add", shared, g.plant(0))])
    g.step("attributes again", [g.attrs_for(m.ids[: (m.count * 9) // 10])])
    g.step("append inside a tile", [("addBatch", g.new_ids(3), [g.plant(1), int(g.rand_rows(1)[0]), g.plant(2)])])
    # seeded steps of the simple kinds, until the sequence has 40 steps
    qi = 0
    while len(g.steps) < 40:
        qi = (qi + 1) % N_QUERIES
        kind = int(rng.integers(0, 7))
        if kind == 0:
            g.step("upsert", [("addBatch", [g.id_at(x) for x in some_rows(2)], [g.plant(qi), int(g.rand_rows(1)[0])])])
        elif kind == 1:
            g.step("append", [("addBatch", g.new_ids(4), [g.plant(qi)] + list(g.rand_rows(3)))])
        elif kind == 2:
            g.step("remove", [("remove", g.top_hit(qi))])
        elif kind == 3:
            g.step("removeBatch", [("removeBatch", [g.top_hit(qi), g.top_hit(qi, rank=1), g.id_at(some_rows(1)[0]), ABSENT_ID, g.top_hit(qi)])])
        elif kind == 4:
            g.step("flag flip", [("setAttributes", [g.top_hit(qi, "A")], None, np.array([1], dtype=np.uint32))])
        elif kind == 5:
            g.step("staged add, upsert", [("add", g.new_ids(1)[0], g.plant(qi)), ("add", g.id_at(some_rows(1)[0]), int(g.rand_rows(1)[0]))])
        else:
            g.step("staged add, setAttributes, reserve", [("add", g.new_ids(1)[0], g.plant(qi)),
                                                          ("setAttributes", [g.top_hit(qi, "A")], None, np.array([1], dtype=np.uint32)),
                                                          ("reserve", g.proto.capacity + 1)])
    return Sequence(name, g.cfg, g.pool, g.queries, g.batch_queries, g.steps), shared


@functools.lru_cache(maxsize=None)
def _built(name):
    return _build(name)


def sequence(name):
    return _built(name)[0]


def shared_id(name):
    """The frame id that two rows of the foreign segment hold."""
    return _built(name)[1]


def blob_of(seq, ids, rows):
    """The MV2V segment of a deserialize_blob op, written by the oracle's serializer."""
    return oracle.mv2v_serialize(seq.metric, seq.pool.rows[np.asarray(rows, dtype=np.int64)], np.asarray(ids, dtype=np.uint64))


# ---------------------------------------------------------------------------------------------------------------------------------
# the certificates

class Margins:
    """Per pool row: the 8-bit key and the bf16 approximate distance to each checked query (float64 models of mirror8_planes_ref and
    predicate_mirror_ref), the row's norm and its bf16 rounding error. margin8 / margin16 of a snapshot are then the formulas of
    mirror8_planes_ref.margin and predicate_mirror_ref.Model.margin over the snapshot's rows, with one difference: the largest norm
    and the largest rounding error are taken over every row the store has held so far, as the engine's running maxima are (they are
    reset only when a mirror starts over) — never smaller than the snapshot's own, so a margin is never overstated."""

    def __init__(self, seq):
        self.seq, self.metric, self.dims = seq, seq.metric, seq.dims
        rows, qs = seq.pool.rows, seq.queries
        cd = R8.Coded(rows, self.metric)
        self.lb8 = np.stack([P8.keys64(q, cd.codes, cd.scale, cd.err, self.metric) for q in qs], axis=1)
        self.exact = np.stack([R8.exact_distances(rows, q, self.metric) for q in qs], axis=1)
        self.norm = np.linalg.norm(rows.astype(np.float64), axis=1)
        x = R8.normalise(rows, self.metric)
        mirror = PM.bf16_rne(x)
        self.err16 = np.linalg.norm(x.astype(np.float64) - mirror.astype(np.float64), axis=1)
        q64 = qs.astype(np.float64)
        self.qn = np.linalg.norm(q64, axis=1)
        approx = mirror.astype(np.float64) @ q64.T
        self.a16 = 1.0 - (approx / self.qn[None, :] if self.metric == COS else approx)
        # running maxima per step
        self.max_norm, self.max_err = [], []
        mn = me = 0.0
        for st in seq.steps:
            mn = max(mn, float(self.norm[st.after.rows].max()))
            me = max(me, float(self.err16[st.after.rows].max()))
            self.max_norm.append(mn)
            self.max_err.append(me)

    def margin8(self, si, qi, k, pred=None):
        snap = self.seq.steps[si].after
        rows = snap.rows[snap.mask(pred)]
        if len(rows) <= KP:
            return -np.inf
        lb = self.lb8[rows, qi]
        cand = np.argsort(lb, kind="stable")[:KP]
        d = np.sort(self.exact[rows[cand], qi])
        return float(lb[cand[-1]] - R8.slack(self.dims, self.metric, self.qn[qi], self.max_norm[si]) - d[k - 1])

    def margin16(self, si, qi, k, pred=None):
        snap = self.seq.steps[si].after
        rows = snap.rows[snap.mask(pred)]
        if len(rows) <= KP:
            return -np.inf
        a = np.partition(self.a16[rows, qi], KP - 1)[KP - 1]
        d = np.partition(self.exact[rows, qi], k - 1)[k - 1]
        eps = PM.finish_eps(self.metric, self.dims, float(np.float32(self.qn[qi])), self.max_norm[si], self.max_err[si])
        return float(a - eps - d)

    def certifies(self, si, qi, k, pred=None):
        """(8-bit, bf16): is the triple in the certifying class of that mirror?"""
        return self.margin8(si, qi, k, pred) >= PM.MARGIN_FLOOR, self.margin16(si, qi, k, pred) >= PM.MARGIN_FLOOR


@functools.lru_cache(maxsize=None)
def margins(name):
    return Margins(sequence(name))
