"""The model behind tests/test_store_sequence_cpu.py and tests/test_store_sequence_gpu.py: one seeded stream of mutations per store,
the store it must leave (numpy only, no engine code), what every derived structure's counter must move by, and the float64 margins of
both mirror certificates.

The engine keeps six structures derived from the f32 store (bf16 mirror, 8-bit code mirror, id -> row table, attribute columns, the
bitmap entries of predicate tickets, the staging area of single adds). Each follows mutations by its own incremental protocol; a
search route that reads one of them gives a wrong answer, with a passing certificate, whenever the structure missed a mutation. The
GPU test replays a Sequence on an engine and, after every step, holds every route to a store rebuilt from this model.

Model      ordered frame ids, rows, ts, flags with the reference's semantics as helpers.OracleEngine has them: upsert by id (first
           row that holds the id), order-preserving remove of that first row, attributes (0, 0) for new rows and after deserialize.
Protocol   the host-side state machines of derived_rows.h, batch_host.inc / api_store.inc / codec.inc and of row_columns.h, restated rule by rule (each
           method names the engine function it restates), so the deltas of "mirror_rows_converted", "idhash_rows_inserted", "mirror8_conversions" and
           "mirror8_rows_converted" over one step (its mutations, then every reader) are predicted, and so the states a step enters are
           tagged with the coverage class they belong to.
Sequence   about 40 steps. A step is one to three mutations with no reader between them (the states the issue lists — an upsert of
           a row the mirror has not converted yet, a removal that renumbers listed dirty rows, growth with rows pending — only exist
           between two readers), then every reader. Every step is planted: an append or upsert puts in a row at cosine
           0.9 - 0.02 j to one of the 4 checked queries (scaled 0.8 .. 1.6 under dot), a removal takes a current top hit, an attribute
           step moves a current top hit across a checked predicate.

The rows of a sequence live in one pool (a row never changes; an upsert points the frame at another pool row), so the per-row terms of
both certificates are computed once per pool row.

The per-row columns of the timeline, grouped and required-term lanes (timestamps and flags, parents, term sets) follow the same
sequences. The store ops, step names and predicted STEP_COUNTERS of the first BASE_STEPS steps are what they were before the columns
joined (BASE_DIGESTS holds a digest of each; neither column op touches a mirror or the id table). The column ops "setParents" and
"setTerms" come from an OVERLAY: a second pass with its own seed per config that replays the finished steps on a fresh model and
protocol and inserts column ops in front of, between and behind a step's store ops, reading the model at that point. Nearly every
step gets one planted setTerms (a current top row of a checked query changes its session term: it crosses R1) and one planted
setParents (the two best rows of a checked query merge into one group, or split); the steps named in _overlay enter the states of
COLUMN_CLASSES. Three states cannot be entered by column ops alone on the first BASE_STEPS steps: a term offset array or a slot column
outgrown by the store (their first upload sizes them for a capacity the store never passes) and a host column emptied by removals
(the parent column reaches to `count` whenever a set extends it). Three TAIL steps behind the old ones enter them: an append past
every device column, the removal of every row under the host columns, the columns set again.

Protocol restates ensure_groups and ensure_terms as it restates the mirrors: "parent_rows_uploaded", "term_rows_uploaded" and
"term_values_uploaded" move over one step by exactly the predicted amount. "group_slots" is no counter but the slot count the last
grouped search saw; it is predicted exactly too, from the restated numbering rule (a root seen keeps its slot, a new one takes the
next, numbering starts over above 2 * count + 16 slots)."""
import functools
import hashlib
import itertools

import numpy as np

import grouped_ref as GR
import mirror8_planes_ref as P8
import mirror8_ref as R8
import oracle
import predicate_mirror_ref as PM
import terms_ref as TR

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
OP_KINDS = ("addBatch", "add", "remove", "removeBatch", "setAttributes", "reserve", "roundtrip", "deserialize_blob", "setParents", "setTerms")
COLUMN_OPS = ("setParents", "setTerms")
L2_CLASSES = ("idhash_realloc", "growth", "remove_batch_plain", "dup_blob")

# the per-row columns
NO_PARENT = int(GR.NO_PARENT)
SESSIONS = (1000, 1001)                      # every initial row holds one of them
TAGS = (2000, 2001, 2002, 2003)              # ... one of these
EVERYBODY = 7                                # ... and this one; then 0 to 6 private terms (PRIVATE0 + a running number)
PRIVATE0 = 100_000
R1 = (SESSIONS[0],)                          # the checked required sets: about half the rows pass R1,
R2 = (SESSIONS[1], TAGS[0])                  # about one in eight R2
REQUIRED = {"R1": R1, "R2": R2}
FOREIGN_ROOT0 = 1 << 40                      # roots the store does not hold
BASE_STEPS = 40                              # the steps that predate the columns; the TAIL steps follow them
OVERLAY = "overlay"                          # fifth element of a setAttributes op the overlay inserted (the only store-op kind it inserts)
COLUMN_COUNTERS = ("parent_rows_uploaded", "group_slots", "term_rows_uploaded", "term_values_uploaded")
NEVER = 1 << 62                              # UploadMark::kNone (row_columns.h)

# sha256 over (name, store ops, predicted STEP_COUNTERS) of the first BASE_STEPS steps, taken on the commit before the columns joined
BASE_DIGESTS = {
    "cos384": "894b393f1149e2a2fd801b8de86da5d7d24df3942d8e3aa5cf23eff24e8f3b70",
    "dot768": "c2afdda81b522a5f8ec530c1eb98e48ba9b58b389a8b3a318000d9902f469dee",
    "l2_100": "5825374a1b075f6c76b53bb4e4895204604ac811a1463c13f35e9692f005432d",
}

# the column states every mirror-capable sequence must enter (tags of Protocol and the overlay)
COLUMN_CLASSES = (
    "terms_first_upload", "terms_same_size_overwrite", "terms_resize_rebuild", "terms_set_behind_column", "terms_append_behind_column",
    "terms_remove_below_column", "terms_remove_behind_column", "terms_remove_batch_straddles_column_end", "terms_value_growth_keeps_prefix",
    "terms_offset_growth_keeps_prefix", "terms_growth_with_stale_below", "terms_all_sets_empty", "terms_emptied", "terms_dropped_by_deserialize",
    "parents_first_set", "parents_column_shorter_than_count", "parents_set_behind_column", "parents_remove_below_column",
    "parents_remove_behind_column", "parents_parent_is_a_held_frame", "parents_parent_frame_removed", "parents_root_table_growth",
    "parents_growth_whole_column", "parents_renumber_from_scratch", "parents_all_no_parent", "parents_emptied", "parents_dropped_by_deserialize",
    "columns_on_shared_id", "staged_pending:setParents", "staged_pending:setTerms", "three_columns_different_lengths",
)
# the l2 store enters all of them but the one that needs the slots of a store of its size to pass 2 * count + 16
L2_COLUMN_CLASSES = tuple(c for c in COLUMN_CLASSES if c != "parents_renumber_from_scratch")
LONG_TIMELINE = {True: None, False: "A"}       # the predicate of the limit-4096 timeline list, by newestFirst
INSERT_POSITIONS = ("insert:front", "insert:between", "insert:behind")


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
        # parent ids (NO_PARENT: the row is its own root) and term sets (sorted tuples), by row
        self.parent, self.terms = [], []

    @property
    def count(self):
        return len(self.ids)

    def find(self, fid):
        try:
            return self.ids.index(fid)
        except ValueError:
            return -1

    def upsert(self, fid, prow):
        """wax_hip_add_batch: an upsert keeps its row's entries in every column; an appended row takes the defaults."""
        i = self.find(fid)
        if i >= 0:
            self.rows[i] = prow
            return i, False
        self.ids.append(fid); self.rows.append(prow); self.ts.append(0); self.fl.append(0)
        self.parent.append(NO_PARENT); self.terms.append(())
        return len(self.ids) - 1, True

    def remove(self, fid):
        """wax_hip_remove / RowColumns::remove_row (and, in one pass, wax_hip_remove_batch): the entries leave with the row."""
        i = self.find(fid)
        if i >= 0:
            for col in (self.ids, self.rows, self.ts, self.fl, self.parent, self.terms):
                del col[i]
        return i

    def set_parents(self, ids, parents):
        """wax_hip_set_parents: ids not held are skipped, entries apply in call order (the last of a repeated id wins), an id two rows
        share names the lower row (idmap.find). Returns the rows named, in call order."""
        hit = []
        for fid, p in zip(ids, parents):
            i = self.find(int(fid))
            if i < 0:
                continue
            self.parent[i] = int(p)
            hit.append(i)
        return hit

    def set_terms(self, ids, sets):
        """wax_hip_set_terms: as set_parents; an entry replaces the row's whole set, duplicates collapse (validate_term_sets), the
        empty set clears. Returns {row: new set} of the rows named."""
        hit = {}
        for fid, s in zip(ids, sets):
            i = self.find(int(fid))
            if i < 0:
                continue
            hit[i] = tuple(sorted(set(int(t) for t in s)))
        for i, s in hit.items():
            self.terms[i] = s
        return hit

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
        # RowColumns::clear: MV2V has no field for any column
        self.parent, self.terms = [NO_PARENT] * len(self.ids), [()] * len(self.ids)

    def has_repeated_ids(self):
        return len(set(self.ids)) != len(self.ids)


class Snapshot:
    """The store after a step, as arrays."""

    def __init__(self, model):
        self.ids = np.array(model.ids, dtype=np.uint64)
        self.rows = np.array(model.rows, dtype=np.int64)
        self.ts = np.array(model.ts, dtype=np.int64)
        self.fl = np.array(model.fl, dtype=np.uint32)
        self.parent = np.array(model.parent, dtype=np.uint64)
        self.terms = list(model.terms)
        self.repeated = model.has_repeated_ids()
        self._term_masks, self._csr = {}, None

    @property
    def count(self):
        return len(self.ids)

    def mask(self, pred, req=None):
        """pred: None (unfiltered), "A", "B" or a bool array per row; req: None or a required term set (terms_ref.pass_set's rule)."""
        if pred is None:
            m = np.ones(self.count, dtype=bool)
        elif isinstance(pred, str):
            m = passing(self.ts, self.fl, **PREDICATES[pred])
        else:
            m = np.asarray(pred, dtype=bool)
        return m & self.term_mask(req) if req else m

    def term_mask(self, req):
        key = tuple(sorted(set(req)))
        if key not in self._term_masks:
            self._term_masks[key] = TR.pass_csr(*self.term_csr(), key)       # (terms_ref.pass_set's answer, without its loop over the rows)
        return self._term_masks[key]

    def term_csr(self):
        """(offsets uint32 [count + 1], values uint32) of the term sets, as terms_ref.csr_of gives them (the sets are sorted and distinct)."""
        if self._csr is None:
            off = np.zeros(self.count + 1, dtype=np.uint32)
            off[1:] = np.cumsum([len(t) for t in self.terms])
            self._csr = off, np.fromiter(itertools.chain.from_iterable(self.terms), dtype=np.uint32, count=int(off[-1]))
        return self._csr

    def has_parents(self):
        return bool((self.parent != GR.NO_PARENT).any())

    def has_terms(self):
        return any(self.terms)


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
        # attribute columns: the host columns' length (RowColumns::attr_rows()) only
        self.a_len = 0
        # parent column (RowColumns::parents().rows()) and what ensure_groups derives: the group mark's two numbers, grp_cap, grp_root_cap,
        # GroupSlots::rows(), GroupSlots' root -> slot map (its size is n_slots())
        self.p_len, self.g_rows, self.g_stale, self.g_cap, self.g_root_cap, self.g_slot_len, self.g_slot_of = 0, 0, NEVER, 0, 0, 0, {}
        # term column: the sets' sizes by row under the host CSR (None: the TermColumn is empty), the term mark's two numbers, both capacities
        self.t_len, self.t_stale, self.t_dev, self.t_off_cap, self.t_val_cap = None, NEVER, 0, 0, 0
        self.tags = set()
        self.moved = set()                                # the lanes ("attrs", "parents", "terms") whose host column a mutation moved or marked

    # -- row_columns.h: RowColumns::clear, and what remove_rows does to a column it leaves empty
    def _parents_replaced(self):
        self.p_len, self.g_rows, self.g_stale, self.g_slot_len, self.g_slot_of = 0, 0, NEVER, 0, {}

    def _terms_replaced(self):
        self.t_len, self.t_stale, self.t_dev = None, NEVER, 0

    def _columns_replaced(self):
        if self.a_len:
            self.moved.add("attrs")
        if self.p_len:
            self.tags.add("parents_dropped_by_deserialize")
            self.moved.add("parents")
        if self.t_len is not None:
            self.tags.add("terms_dropped_by_deserialize")
            self.moved.add("terms")
        self.a_len = 0
        self._parents_replaced()
        self._terms_replaced()

    # -- row_columns.h: RowColumns::remove_row (wax_hip_remove) and remove_rows (wax_hip_remove_batch)
    def _columns_remove(self, rem):
        """rem: the rows that leave, ascending and distinct."""
        if self.p_len:
            below = sum(1 for r in rem if r < self.p_len)
            if below:
                self.tags.add("parents_remove_below_column")
                self.moved.add("parents")
            if rem[-1] >= self.p_len:
                self.tags.add("parents_remove_behind_column")
            self.p_len -= below
            if self.p_len == 0:
                self._parents_replaced()
                self.tags.add("parents_emptied")
            else:
                self.g_stale = min(self.g_stale, rem[0])          # remove_rows: a row behind the column shifts its slot entry all the same
        if self.t_len is not None:
            nt = len(self.t_len)
            if rem[0] < nt:
                self.tags.add("terms_remove_below_column")
                self.moved.add("terms")
                gone = set(rem)
                self.t_len = [n for r, n in enumerate(self.t_len) if r not in gone]
            if rem[-1] >= nt:
                self.tags.add("terms_remove_behind_column")
                if len(rem) > 1 and rem[0] < nt:
                    self.tags.add("terms_remove_batch_straddles_column_end")
            if not self.t_len:
                self._terms_replaced()
                self.tags.add("terms_emptied")
            else:
                self.t_stale = min(self.t_stale, rem[0])          # remove_rows marks while the column exists
        below = sum(1 for r in rem if r < self.a_len)
        if below:
            self.moved.add("attrs")
        self.a_len -= below

    # -- api_grouped.inc: wax_hip_set_parents (RowColumns::set_parent)
    def set_parents(self, rows):
        """rows: the store rows the entries named, in call order."""
        if self.pend:
            self.tags.add("staged_pending:setParents")
        if not rows:
            return
        for r in rows:
            if self.p_len <= r:
                self.tags.add("parents_set_behind_column" if self.p_len else "parents_first_set")
                self.p_len = self.count                           # everything up to it was its own root
        self.g_stale = min(self.g_stale, min(rows))               # set_parent marks every row it sets
        self.moved.add("parents")

    # -- api_terms.inc: wax_hip_set_terms (row_columns.h: finish_term_rows, TermColumn::commit, RowColumns::commit_terms)
    def set_terms(self, sizes):
        """sizes: {store row: size of its new set} (one entry per row: the last of a repeated id has won)."""
        if self.pend:
            self.tags.add("staged_pending:setTerms")
        if not sizes:
            return
        rows = sorted(sizes)
        old_rows = len(self.t_len) if self.t_len is not None else 0
        resized = [r for r in rows if not (r < old_rows and sizes[r] == self.t_len[r])]
        if resized:
            # the CSR is rebuilt from the lowest resized row to the column's end: the old one's, or the highest row set behind it
            if self.t_len is None:
                self.t_len = []
            elif rows[-1] >= old_rows:
                self.tags.add("terms_set_behind_column")
            self.t_len += [0] * (max(old_rows, rows[-1] + 1) - old_rows)
            for r in rows:
                self.t_len[r] = sizes[r]
            self.tags.add("terms_resize_rebuild")
        else:
            self.tags.add("terms_same_size_overwrite")            # values change, offsets do not
        self.t_stale = min(self.t_stale, rows[0])                 # commit_terms marks rows.front()
        self.moved.add("terms")

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

    # -- derived_rows.h: what DerivedRows' operations do to the code mirror: RowFill::appended / RowFill::restart
    def _c8_append(self):
        self.c_valid = False

    def _c8_stale(self):
        self.c_valid, self.c_stale = False, True

    # -- derived_rows.h: DerivedRows::overwritten
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
        self.h_valid = False                              # DerivedRows::appended
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

    # -- api_store.inc: wax_hip_remove + batch_host.inc: mirror_follow_remove + derived_rows.h: DerivedRows::removed(row, followed)
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
        self._columns_remove([idx])
        self.count -= 1

    # -- api_store.inc: wax_hip_remove_batch + batch_host.inc: compact_removed_rows + derived_rows.h: DerivedRows::removed(rem, m, followed)
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
        self._columns_remove(list(rem))
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

    # -- api_predicate.inc: wax_hip_set_attributes (RowColumns::set_attributes)
    def set_attributes(self, rows=()):
        """rows: the store rows the entries named."""
        if self.pend:
            self.tags.add("staged_pending:setAttributes")
        for r in rows:
            if self.a_len <= r:
                self.a_len = self.count                           # the columns end below this row: everything up to it was (0, 0)
        if len(rows):
            self.moved.add("attrs")

    def reserve(self, rows):
        if self.pend:
            self.tags.add("staged_pending:reserve")
        self._reserve_rows(rows)

    # -- codec.inc: wax_hip_deserialize (DerivedRows::replaced; capacity only grows, to the segment's rows exactly)
    def deserialize(self, n, kind):
        if self.pend:
            self.tags.add("staged_pending:" + kind)
        self.m_stale, self.m_dirty, self.m_rows = True, [], 0
        self.h_valid, self.h_stale, self.h_rows = False, True, 0
        self._c8_stale()
        self._columns_replaced()                          # RowColumns::clear
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

    # -- the column readers: ensure_groups (with GroupSlots::number of row_columns.h; every grouped search) and ensure_terms (every term search on a device bitmap). Both run at
    # -- least once per step on the store the step left; every later call of the step finds the columns current and uploads nothing.
    def read_columns(self, model):
        """The deltas of groupStats()["parent_rows_uploaded"], termStats()["term_rows_uploaded"] and ["term_values_uploaded"] over the
        step, and groupStats()["group_slots"] after it (the slot count the step's last grouped search saw)."""
        count, out = self.count, dict.fromkeys(COLUMN_COUNTERS, 0)
        assert count == model.count
        # ensure_groups
        if self.p_len == 0:
            out["group_slots"] = count                                # a store without parents: slot = row
        else:
            frm = min(self.g_rows, self.g_stale, count)
            if frm < count or self.g_slot_len != count:
                def number_from(r0):
                    for r in range(r0, count):
                        p = model.parent[r] if r < self.p_len else NO_PARENT
                        self.g_slot_of.setdefault(p if p != NO_PARENT else model.ids[r], len(self.g_slot_of))
                number_from(frm)
                self.g_slot_len = count
                if len(self.g_slot_of) > 2 * count + 16:              # removals left most slots without a row: number from scratch
                    self.g_slot_of = {}
                    frm = 0
                    number_from(0)
                    self.tags.add("parents_renumber_from_scratch")
                if self.g_cap < count:                                # growth: the column is sent again whole
                    if self.g_cap:
                        self.tags.add("parents_growth_whole_column")
                    self.g_cap = max(self.capacity, count)
                    frm = 0
                if self.g_root_cap < len(self.g_slot_of):
                    if len(self.g_slot_of) > 1024:
                        self.tags.add("parents_root_table_growth")
                    self.g_root_cap = 1024
                    while self.g_root_cap < len(self.g_slot_of):
                        self.g_root_cap *= 2
                out["parent_rows_uploaded"] = count - frm
            self.g_rows, self.g_stale = count, NEVER
            out["group_slots"] = len(self.g_slot_of)
            if self.p_len < count:
                self.tags.add("parents_column_shorter_than_count")
            if all(p == NO_PARENT for p in model.parent[:self.p_len]):
                self.tags.add("parents_all_no_parent")
        # ensure_terms (an empty host column: the search is decided on the host and nothing is touched)
        if self.t_len is not None:
            host_rows, off = len(self.t_len), np.concatenate([[0], np.cumsum(self.t_len, dtype=np.int64)])
            total = int(off[-1])
            host_off = lambda r: int(off[min(r, host_rows)])
            frm = min(self.t_dev, self.t_stale, count)
            current = frm == count and self.t_dev == count and self.t_stale == NEVER
            val_need = ((total + 3) & ~3) + 4
            if self.t_off_cap < count + 1 or self.t_val_cap < val_need:
                # the rows that were current are kept by a device copy, the rest is uploaded
                if self.t_off_cap == 0:
                    self.tags.add("terms_first_upload")
                keep = 0 if self.t_off_cap == 0 else min(frm, self.t_off_cap - 1)
                if keep > 0 and self.t_stale < min(self.t_dev, count):
                    self.tags.add("terms_growth_with_stale_below")
                if self.t_off_cap < count + 1:
                    if keep > 0 and self.t_stale == NEVER and frm == self.t_dev:
                        self.tags.add("terms_offset_growth_keeps_prefix")
                    self.t_off_cap = max(self.capacity, count) + 1
                if self.t_val_cap < val_need:
                    if keep > 0:
                        self.tags.add("terms_value_growth_keeps_prefix")
                    self.t_val_cap = max(self.t_val_cap * 2, 1024)      # the value array doubles from 1024
                    while self.t_val_cap < val_need:
                        self.t_val_cap *= 2
                self.t_dev, frm, current = keep, min(frm, keep), False
            if not current:
                out["term_rows_uploaded"] = count - frm
                out["term_values_uploaded"] = total - host_off(frm)
            self.t_dev, self.t_stale = count, NEVER
            if host_rows < count:
                self.tags.add("terms_append_behind_column")
            if total == 0:
                self.tags.add("terms_all_sets_empty")
        lens = (self.a_len, self.p_len, len(self.t_len) if self.t_len is not None else 0)
        if min(lens) > 0 and len(set(lens)) == 3 and max(lens) < count:
            self.tags.add("three_columns_different_lengths")
        return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the sequence

class Step:
    def __init__(self, name, ops):
        self.name, self.ops = name, ops
        self.tags, self.after, self.counters = set(), None, None
        self.column_counters, self.moved = None, set()    # COLUMN_COUNTERS as predicted; the lanes whose host column the ops moved or marked
        self.term_column = False                          # does the host term column exist at the step's readers (else: decided on the host)
        self.attr_column = False                          # ... and the attribute columns (else a predicate is decided on the host: every row is (0, 0))


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

    def top(self, snap, qi, pred, k=10, req=None):
        """The float64 top-k of query qi among the rows that pass `pred` (and hold every term of `req`): (frame ids, pool rows), best
        first, row order breaks ties."""
        rows = np.flatnonzero(snap.mask(pred, req))
        d = self.pool.exact[snap.rows[rows], qi]
        order = np.lexsort((rows, d))[:k]
        return snap.ids[rows[order]], snap.rows[rows[order]]

    def grouped(self, snap, qi, pred, limit=10, per_group=3):
        """The float64 grouped answer of query qi (grouped_ref.grouped_model's rule on float64 distances): a tuple of
        (root, the store rows of its best members) by (best distance, root)."""
        rows = np.flatnonzero(snap.mask(pred))
        if len(rows) == 0:
            return ()
        d = self.pool.exact[snap.rows[rows], qi]
        order = np.lexsort((rows, d))
        rows, d = rows[order], d[order]
        roots = GR.roots_of(snap.parent, snap.ids)[rows]
        uniq, first = np.unique(roots, return_index=True)
        best = np.lexsort((uniq, d[first]))[:limit]
        return tuple((int(uniq[g]), tuple(int(r) for r in rows[roots == uniq[g]][:per_group])) for g in best)

    def timeline(self, snap, limit, newest, pred):
        """timeline_ref.timeline_model's rule, vectorised: (frame ids, timestamps)."""
        rows = np.flatnonzero(snap.mask(pred))
        ts = snap.ts[rows]
        order = np.lexsort((rows, snap.ids[rows], -ts if newest else ts))[:limit]
        return snap.ids[rows[order]], ts[order]

    def lane_answers(self, snap, lane):
        """What the checked queries of one lane's reader return on the model (test_store_sequence_cpu.py: the lanes' teeth)."""
        if lane == "attrs":
            return [tuple(map(tuple, self.timeline(snap, limit, newest, pred))) for newest in (True, False) for pred in (None, "A", "B")
                    for limit in (10, 4096 if pred == LONG_TIMELINE[newest] else 300)]
        if lane == "parents":
            out = [self.grouped(snap, qi, pred) for qi in range(N_QUERIES) for pred in (None, "A", "B")]
            return out + [self.grouped(snap, 0, None, 1024, 8)]
        return [tuple(map(tuple, self.top(snap, qi, pred, 10, req))) for req in (R1, R2) for qi in range(N_QUERIES) for pred in (None, "A")]


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
        self.begin()
        for op in st.ops:
            self.apply(op)
        if then is not None:
            more = then()
            for op in more:
                self.apply(op)
            st.ops += more
        return self.finish(st)

    def begin(self):
        self.proto.tags, self.proto.moved = set(), set()

    def finish(self, st):
        """The readers: the step's counters, tags and the store it left."""
        st.counters = self.proto.read()
        st.column_counters = self.proto.read_columns(self.model)
        st.tags = set(self.proto.tags) | getattr(self, "_extra_tags", set())
        st.moved = set(self.proto.moved)
        st.term_column, st.attr_column = self.proto.t_len is not None, self.proto.a_len > 0
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
            if int(op[1]) in m.parent and m.find(int(op[1])) >= 0:
                self.tag("parents_parent_frame_removed")          # the children keep their root
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
            p.set_attributes([i for i in (m.find(int(fid)) for fid in op[1]) if i >= 0])
            m.set_attributes(op[1], op[2], op[3])
        elif kind == "setParents":
            held = set(m.ids)
            if any(int(q) in held for q in op[2]):
                self.tag("parents_parent_is_a_held_frame")
            p.set_parents(m.set_parents(op[1], op[2]))
        elif kind == "setTerms":
            p.set_terms({i: len(s) for i, s in m.set_terms(op[1], op[2]).items()})
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
    assert len(g.steps) == BASE_STEPS
    _overlay(g, g.steps, shared)
    return Sequence(name, g.cfg, g.pool, g.queries, g.batch_queries, g.steps), shared


def _ids_named(ops):
    out = set()
    for op in ops:
        if op[0] in ("addBatch", "removeBatch"):
            out |= {int(i) for i in op[1]}
        elif op[0] in ("add", "remove"):
            out.add(int(op[1]))
    return out


def _overlay(g, base, shared):
    """The column ops: replays the finished steps on a fresh model and protocol (the store ops, their counters and tags must come out
    as they were), inserts setParents / setTerms in front of, between and behind them, then appends the three tail steps."""
    orng = np.random.default_rng(g.cfg["seed"] + 500)
    g.model, g.proto, g.steps, g.rng = Model(), Protocol(g.cfg["mirror"]), [], orng
    m, mirror = g.model, g.cfg["mirror"]
    n_roots = max(8, g.n0 // 8)
    fresh = {"private": PRIVATE0, "root": 0, "floor": 0}

    def private(k):
        fresh["private"] += k
        return list(range(fresh["private"] - k, fresh["private"]))

    def new_root():
        fresh["root"] += 1
        return (1 << 41) + fresh["root"]

    def unique_ids():
        return list(dict.fromkeys(m.ids))

    def full_terms(ids, extra=()):
        """A session term, a tag, the term every row holds and 0 to 6 private ones per frame."""
        sets = [[SESSIONS[int(orng.integers(0, 2))], TAGS[int(orng.integers(0, 4))], EVERYBODY] + private(int(orng.integers(0, 7))) for _ in ids]
        return ("setTerms", [int(i) for i in ids] + [int(i) for i, _ in extra], sets + [list(s) for _, s in extra])

    def full_parents(ids, extra=()):
        """About four in five get one of n / 8 foreign roots, one in twenty a held frame's id, the rest none."""
        held, par = list(m.ids), []
        for x in orng.random(len(ids)):
            par.append(FOREIGN_ROOT0 + int(orng.integers(0, n_roots)) if x < 0.8 else int(held[int(orng.integers(0, len(held)))]) if x < 0.85 else NO_PARENT)
        return ("setParents", [int(i) for i in ids] + [int(i) for i, _ in extra], par + [int(p) for _, p in extra])

    def ranked(qi, below, avoid, k=10):
        """The best rows of query qi that lie under a column of `below` rows and are not named by the step's later store ops."""
        rows = np.array(m.rows, dtype=np.int64)
        order = np.lexsort((np.arange(len(rows)), g.pool.exact[rows, qi]))
        return [int(r) for r in order[:k] if fresh["floor"] <= r < below and m.ids[r] not in avoid and m.ids[r] != shared]

    def tooth_terms(qi, avoid, resize):
        """A current top row of query qi changes its session term: it crosses R1."""
        below = len(g.proto.t_len) if g.proto.t_len is not None else m.count
        r = ranked(qi, below, avoid)[0]
        cur = list(m.terms[r])
        if SESSIONS[0] in cur:
            cur[cur.index(SESSIONS[0])] = SESSIONS[1]
        elif SESSIONS[1] in cur:
            cur[cur.index(SESSIONS[1])] = SESSIONS[0]
        else:
            cur += [SESSIONS[0], TAGS[0], EVERYBODY]
        if resize:
            cur += private(1 + int(orng.integers(0, 3)))
        return ("setTerms", [m.ids[r]], [cur])

    def tooth_parents(qi, avoid):
        """The two best rows of query qi merge into one group where they lead two, and split where they share one."""
        a, b = ranked(qi, g.proto.p_len or m.count, avoid)[:2]
        root = lambda r: m.parent[r] if m.parent[r] != NO_PARENT else m.ids[r]
        return ("setParents", [m.ids[b]], [root(a) if root(a) != root(b) else new_root()])

    def emit(name, ops, plan):
        """plan: where ("front", "between", "behind") -> callables that return the column ops to insert there."""
        st = Step(name, [])
        g.begin()

        def insert(where):
            for make in plan.get(where, ()):
                for op in make():
                    g.apply(op)
                    st.ops.append(op)
                    g.tag("insert:" + where)
        insert("front")
        for j, op in enumerate(ops):
            if j == 1:
                insert("between")
            g.apply(op)
            st.ops.append(op)
        insert("behind")
        return g.finish(st)

    names = [st.name for st in base]
    dup = names.index("two rows, one id")
    pure = (8, 10, 12)                                   # no column op: an unchanged column uploads nothing; deserialize drops the columns
    assert [names[i] for i in pure] == ["flag flip", "ts move", "serialize, deserialize"] and names[13] == "attributes again"
    for si, bst in enumerate(base):
        ops, plan = list(bst.ops), {"front": [], "between": [], "behind": []}
        named = _ids_named(ops)
        where = ("behind", "front", "between")[si % 3]
        if where == "between" and len(ops) < 2:
            where = "front"
        if si == 4:
            where = "between"                             # staged single adds are pending in front of both column ops
        if len(named) > 200 or si == dup:
            where = "behind"
        avoid = set() if where == "behind" else named if where == "front" else _ids_named(ops[1:])
        teeth = [lambda: [tooth_terms(si % N_QUERIES, avoid, resize=si % 2 == 0)], lambda: [tooth_parents((si + 1) % N_QUERIES, avoid)]]
        if si == 0:
            # every initial row gets its term set and its parent: the first upload of both columns
            plan["behind"] = [lambda: [full_terms(m.ids), full_parents(m.ids)]]
        elif si in pure:
            pass
        elif si == 3:
            # the row the step before planted for query 0, not the last it appended: the term column then ends four rows behind the
            # attribute columns, the parent column at the count before this step's append
            plan["front"] = [lambda: [("setTerms", [m.ids[g.n0 + 3]], [[SESSIONS[0], TAGS[1], EVERYBODY]]),
                                      ("setParents", [m.ids[g.n0 + 3]], [FOREIGN_ROOT0 + 1])]]
            plan[where] += teeth
        elif si == 5:
            # two top rows become children of the frame this step removes: they keep their root
            gone = int(ops[2][1])
            plan["front"] = [lambda: [("setParents", [m.ids[r] for r in ranked(1, g.proto.p_len, named)[:2]], [gone, gone])]]
            plan[where] += [teeth[0]]
        elif si == 13:
            # behind the deserialize of the step before: both columns exist again and hold nothing
            def nothing():
                ids = unique_ids()[::max(1, m.count // 63)] + [m.ids[-1]]
                return [("setTerms", ids, [[] for _ in ids]), ("setParents", ids, [NO_PARENT] * len(ids))]
            plan["behind"] = [nothing]
        elif si == 14:
            plan["front"] = [lambda: [full_terms(m.ids), full_parents(m.ids)]]
        elif si == 15:
            # sets in the upper part of the store grow until the value array must: the rows below the lowest of them stay on the device
            def grow_values():
                p = g.proto
                need, ids, sets = p.t_val_cap + 1 - sum(p.t_len), [], []
                r = (len(p.t_len) * 3) // 5
                while need > 0:
                    k = TR.MAX_PER_ROW - 4 - len(m.terms[r])
                    ids.append(m.ids[r]); sets.append(list(m.terms[r]) + private(k))
                    need -= k
                    r += 1
                tooth = tooth_terms((si + 2) % N_QUERIES, set(), resize=False)      # (the op has its own tooth, on a row below them)
                return [("setTerms", tooth[1] + ids, tooth[2] + sets)]
            fresh["floor"] = 1                            # (row 0 is named by no op of this step: a prefix stays on the device)
            plan[where] += teeth
            plan["behind"] += [grow_values]
        elif si == dup:
            # behind the deserialize: every frame again, and the timestamp, parent and terms of the id two rows share (its last entry wins,
            # and names the lower row)
            def shared_columns():
                g.tag("columns_on_shared_id")
                return [full_terms(unique_ids(), [(shared, [SESSIONS[0], TAGS[0], EVERYBODY] + private(2))]),
                        full_parents(unique_ids(), [(shared, FOREIGN_ROOT0 + 3)]),
                        ("setAttributes", [shared], np.array([3000], dtype=np.int64), np.array([0], dtype=np.uint32), OVERLAY)]
            plan["behind"] = [shared_columns]
        elif mirror and si in (23, 25):
            # every row its own fresh root, twice: the slots pass 1024, then 2 * count + 16
            plan["behind"] = [teeth[0], lambda: [("setParents", unique_ids(), [new_root() for _ in unique_ids()])]]
        elif mirror and si in (24, 26):
            plan["behind"] = [teeth[0], lambda: [full_parents(unique_ids())]]
        else:
            plan[where] += teeth
        if "dup_upsert_second_row" in bst.tags:
            g.tag("dup_upsert_second_row")                # (named by _build, not by a rule)
        st = emit(bst.name, ops, plan)
        fresh["floor"] = 0
        assert st.counters == bst.counters and bst.tags <= st.tags, (si, bst.name, st.counters, bst.counters)
        assert np.array_equal(st.after.ids, bst.after.ids) and np.array_equal(st.after.rows, bst.after.rows), (si, bst.name)
    # the tail: an append past the term offsets and the slot column (both current), the removal of every row under the three host
    # columns, the columns again
    p, under = g.proto, m.count
    n = max(p.t_off_cap, p.g_cap) - m.count + 16
    vec = list(g.rand_rows(n))
    vec[3], vec[n // 2], vec[n - 2], vec[5] = g.plant(0), g.plant(1), g.plant(2), g.plant(3)
    emit("append past every device column", [("addBatch", g.new_ids(n), vec)], {})
    emit("removal of every row under the columns", [("removeBatch", [int(i) for i in m.ids[:under]])], {})
    emit("columns again", [g.attrs_for(m.ids)], {"behind": [lambda: [full_terms(m.ids), full_parents(m.ids)]]})


def grouped_answer(keys, parents, frame_ids, passing, limit, per_group, by_key=None, root_index=None):
    """grouped_ref.grouped_model without its loop over the rows: the same Answer, array for array (test_store_sequence_cpu.py).
    by_key: np.argsort(keys, kind="stable"); root_index: np.unique(roots_of(parents, frame_ids), return_inverse=True) — where the
    caller asks several answers on the same keys or the same store."""
    keys, per_group = np.asarray(keys, dtype=np.int64), max(1, int(per_group))
    uniq, index = root_index if root_index is not None else np.unique(GR.roots_of(parents, frame_ids), return_inverse=True)
    part = keys != GR.KEY_PAD
    if passing is not None:
        part &= np.asarray(passing, dtype=bool)
    if by_key is None:
        by_key = np.argsort(keys, kind="stable")
    order = by_key[part[by_key]]                                    # the rows that take part, best first
    group, n = index[order], len(order)
    first = np.full(len(uniq), n, dtype=np.int64)
    first[group[::-1]] = np.arange(n - 1, -1, -1)                   # a root's first row in key order is its best (the lowest place wins)
    present = np.flatnonzero(first < n)
    bits = keys[order[first[present]]] >> 32
    best = present[np.lexsort((uniq[present], bits))[:max(0, int(limit))]]      # (distance bits, root id as unsigned)
    g = len(best)
    place = np.full(len(uniq), -1, dtype=np.int64)
    place[best] = np.arange(g)
    chosen = np.flatnonzero(place[group] >= 0)                      # the rows of the groups that made it, still best first
    slot = place[group[chosen]]
    by_slot = np.argsort(slot, kind="stable")                       # key order survives inside a group
    slot_sorted = slot[by_slot]
    rank = np.arange(len(slot_sorted)) - np.searchsorted(slot_sorted, np.arange(g))[slot_sorted]
    take = rank < per_group
    members = np.full((g, per_group), GR.KEY_PAD, dtype=np.int64)
    members[slot_sorted[take], rank[take]] = keys[order[chosen[by_slot[take]]]]
    counts = (members != GR.KEY_PAD).sum(axis=1).astype(np.uint32)
    return GR.Answer(uniq[best].astype(np.uint64), (keys[order[first[best]]] >> 32).astype(np.int32), members, counts)


def model_apply(m, op):
    """One op on a Model alone (what _Gen.apply does to it)."""
    kind = op[0]
    if kind == "addBatch":
        for fid, prow in zip(op[1], op[2]):
            m.upsert(int(fid), int(prow))
    elif kind == "add":
        m.upsert(int(op[1]), int(op[2]))
    elif kind == "remove":
        m.remove(int(op[1]))
    elif kind == "removeBatch":
        for fid in op[1]:
            m.remove(int(fid))
    elif kind == "setAttributes":
        m.set_attributes(op[1], op[2], op[3])
    elif kind == "setParents":
        m.set_parents(op[1], op[2])
    elif kind == "setTerms":
        m.set_terms(op[1], op[2])
    elif kind == "roundtrip":
        m.replace(m.ids, m.rows)
    elif kind == "deserialize_blob":
        m.replace(op[1], op[2])
    else:
        assert kind == "reserve", kind


def store_ops(step):
    """A step's ops without what the overlay inserted."""
    return [op for op in step.ops if op[0] not in COLUMN_OPS and not (len(op) == 5 and op[4] == OVERLAY)]


def _canonical(x):
    if isinstance(x, np.ndarray):
        return [int(v) for v in x.reshape(-1)]
    if isinstance(x, (list, tuple)):
        return [_canonical(v) for v in x]
    return x if x is None or isinstance(x, str) else int(x)


def digest(steps):
    """sha256 over (name, store ops, predicted STEP_COUNTERS) of the steps: BASE_DIGESTS."""
    h = hashlib.sha256()
    for st in steps:
        h.update(repr((st.name, _canonical(store_ops(st)), sorted(st.counters.items()))).encode())
    return h.hexdigest()


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

    def margin16(self, si, qi, k, pred=None, req=None):
        """pred: None, a named predicate or any row mask (a bool per row); req: a required term set folded into it."""
        snap = self.seq.steps[si].after
        rows = snap.rows[snap.mask(pred, req)]
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
