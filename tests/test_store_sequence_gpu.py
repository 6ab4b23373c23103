"""Every search route held to a rebuilt store across one seeded sequence of mutations per store (store_sequence_ref.py).

After every step (one to three mutations, no reader between them) every reader below runs on the engine under test, in an order
rotated by the step index, so each reader is in turn the first to meet the mutation. Expected answers:
  (a) a fresh engine built from the model's rows with one addBatch (one deserialize where two rows share a frame id: addBatch cannot
      express that) and one setAttributes, read with "scan_mirror" 0 and "filter_device_min" -1; filtered answers are read as
      searchFiltered(frameIds = the ids the numpy predicate model passes). Every reader's ids and scores are array_equal to it.
  (b) the float64 oracle on the model's matrix: the fresh engine's answers under helpers.assert_parity.
Also after every step: count, serialize() byte for byte, getAttributes of every id; and the deltas of "mirror_rows_converted",
"idhash_rows_inserted", "mirror8_conversions" and "mirror8_rows_converted" over the step equal Protocol's prediction, so a silent whole
rebuild cannot stand in for the incremental path. Fallback counters are zero wherever test_store_sequence_cpu.py has shown the
float64 margin of that mirror to be >= MARGIN_FLOOR; elsewhere only equality is asserted.

The handle of three shards runs the readers a handle serves (searchMany refuses one). Each shard certifies on its own rows and keeps
its own structures, which Protocol does not model: on the handle the answers, count, serialize and attributes are asserted, the
counters are not. The l2 store (100 dimensions) has no mirror and no masked scan: the counters show that those readers fell back.

The timeline, grouped and required-term lanes are three more readers (thirteen in the rotation), each held to its lane's model on the
snapshot's columns: read_timeline to Sequence.timeline (timeline_ref.timeline_model's rule), timelineDevice on a side stream included;
read_grouped to grouped_answer (grouped_ref.grouped_model's rule) on the exact row keys the fresh engine gives, the fresh engine's own
searchGrouped included, on the fused scan and, once per step, under "force_general" on the column route; read_terms to (a) with the
required set folded into the mask (terms_ref.pass_set's rule), on the gather route, the masked f32 scan and the masked bf16 pass, with
the exact counter deltas of every call. test_store_sequence_cpu.py proves the three vectorised models equal to the lane models. To
keep a step short the three readers ask fewer queries than the other ten: read_grouped and read_terms ask one of the four checked
queries per step and predicate (or required set), each in its turn, beginning with the query whose top rows the step's planted
setParents / setTerms names; read_timeline asks limit 1 only without a predicate, its limit-4096 list once per order (the newest
under no predicate, the oldest under A) and timelineDevice once per order and predicate; getTerms reads every 16th id of an op that
names the whole store. Every route, class and step is read. After every step getParents of every id and getTerms of
every id a column op named are the model's, and "parent_rows_uploaded", "term_rows_uploaded", "term_values_uploaded" move by, and
"group_slots" stands at, what Protocol.read_columns predicts from the restated ensure_groups and ensure_terms: exactly, the numbering
rule included. The handle runs the three readers without timelineDevice and with one member per group (it refuses more), answers and
get-calls only. The three readers and the column counters found nothing: every answer and every prediction held as first written.

What the sequence found (fixed in this commit): after `deserialize` of a segment in which two rows hold one frame id, `remove` of that
id took the lower row and dropped the id from the host map, so the surviving row could no longer be addressed: a second `remove` was a
no-op, an upsert appended a third row, `getAttributes` reported the frame missing and the host probe of an allow-list disagreed with
the device table. Exposed by the step "upsert of the shared id" (count and serialize) and, one step earlier, by getAttributes."""
import time

import numpy as np
import pytest

import grouped_ref as GR
import oracle
import store_sequence_ref as S
import timeline_ref as TL
from helpers import assert_parity

pytestmark = pytest.mark.gpu

PARITY_MARGIN = 8
STEP_COUNTERS = ("mirror_rows_converted", "idhash_rows_inserted", "mirror8_conversions", "mirror8_rows_converted")
TERM_ROUTES = ((1, 0), (2, 0), (2, 2))                  # ("predicate_route", "predicate_mirror"): the gather, the masked f32 scan, the masked bf16 pass
PREDICATE_COUNTERS = ("predicate_gather_searches", "predicate_masked_scans", "predicate_mirror_scans", "predicate_mirror_fallbacks")
METRIC_NAMES = ("cosine", "dot", "l2")
SWITCHES = {"scan_mirror": 0, "mirror_bits": 16, "mirror_share": 0, "filter_device_min": -1, "predicate_route": 0, "predicate_mirror": 0}


@pytest.fixture(scope="module")
def wax(hip_lib):
    import wax_amd
    if hip_lib.wax_hip_device_count() == 0:
        pytest.skip("no HIP device on this host: the gpu-marked tests run on the MI355X box (pytest -m gpu)")
    assert hip_lib.wax_hip_available() == 1, "a HIP device is visible but it is not gfx950: the HIP path needs an MI355X"
    return wax_amd


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def allowed(fid):
    """The allow-list of the frameIds readers: about two frames in three, by a rule on the id (so new frames fall on both sides)."""
    return (int(fid) * 2654435761 >> 7) % 3 != 0


def same_grouped(got, exp):
    """searchGrouped's five arrays against (roots, score bits, member ids, member score bits, counts)."""
    roots, scores, mids, mscores, counts = got
    return (np.array_equal(roots, exp[0]) and np.array_equal(scores.view(np.int32), exp[1]) and mids.shape == exp[2].shape and np.array_equal(mids, exp[2])
            and np.array_equal(mscores.view(np.int32), exp[3]) and np.array_equal(counts, exp[4]))


def set_terms_csr(eng, ids, begin, lens, values):
    """wax_hip_set_terms on CSR arrays as they are (HIPVectorEngine.setTerms builds them from Python sets: too slow once per step)."""
    import ctypes
    from wax_amd.errors import raise_for_status
    ids, begin = np.ascontiguousarray(ids, dtype=np.uint64), np.ascontiguousarray(begin, dtype=np.uint64)
    lens, values = np.ascontiguousarray(lens, dtype=np.uint32), np.ascontiguousarray(values, dtype=np.uint32)
    u64, u32, applied = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint64(0)
    raise_for_status(eng._lib.wax_hip_set_terms(eng._h, ids.ctypes.data_as(u64), begin.ctypes.data_as(u64), lens.ctypes.data_as(u32),
                                                values.ctypes.data_as(u32) if values.size else None, int(values.size), int(ids.size), ctypes.byref(applied)))
    return int(applied.value)


class Reference:
    """(a) and (b) for the store after one step; every answer is computed once."""

    def __init__(self, wax, seq, snap):
        self.seq, self.snap = seq, snap
        self.matrix = seq.matrix(snap)
        self.eng = wax.HIPVectorEngine(metric=wax.VectorMetric(seq.metric), dimensions=seq.dims)
        if snap.repeated:
            self.eng.deserialize(oracle.mv2v_serialize(seq.metric, self.matrix, snap.ids))
        else:
            self.eng.addBatch(snap.ids, self.matrix)
        _, first = np.unique(snap.ids, return_index=True)          # a shared id names its lower row
        first.sort()
        assert self.eng.setAttributes(snap.ids[first], snap.ts[first], snap.fl[first]) == len(first)
        # the two columns, where the model's hold anything; by descending row, so that the last entry of a shared id names its lower row
        if snap.has_parents():
            assert self.eng.setParents(snap.ids[::-1], snap.parent[::-1]) == snap.count
        if snap.has_terms():
            off, val = snap.term_csr()
            assert set_terms_csr(self.eng, snap.ids[::-1], off[:-1][::-1], np.diff(off)[::-1], val) == snap.count
        self.eng.setTuning("scan_mirror", 0)
        self.eng.setTuning("filter_device_min", -1)
        self.allow = np.array([i for i in snap.ids if allowed(i)] + [S.ABSENT_ID], dtype=np.uint64)
        self.in_allow = np.isin(snap.ids, self.allow)
        self.short = snap.ids[::max(1, snap.count // 300)][:300]          # a short allow-list of held ids: staged on the host
        self.in_short = np.isin(snap.ids, self.short)
        self.cache, self.oracle_cache, self.keys, self.by_key, self.root_index, self.grouped_cache = {}, {}, None, {}, None, {}

    def close(self):
        self.eng.close()

    def mask(self, pred, listed, req=None):
        """listed: False, True (the long allow-list) or "short"; req: a required term set (terms_ref.pass_set on the model's sets)."""
        m = self.snap.mask(pred, req)
        return m & (self.in_short if listed == "short" else self.in_allow) if listed else m

    def answer(self, qi, k, pred=None, listed=False, req=None):
        """qi indexes the 32 batch queries; the first four are the checked ones (the only ones asked with a filter, and held to the oracle)."""
        key = (qi, k, pred, listed, req)
        if key not in self.cache:
            q = self.seq.batch_queries[qi]
            if pred is None and not listed and req is None:
                got = self.eng.searchArrays(q, k)
            else:
                got = self.eng.searchFiltered(q, k, frameIds=self.snap.ids[self.mask(pred, listed, req)])
            self.cache[key] = got
            if qi < S.N_QUERIES:
                self.parity(qi, k, pred, listed, got, req)
        return self.cache[key]

    def row_keys(self):
        """Every row's exact key to the four checked queries, by row (test_grouped_gpu.row_keys): [query, row]."""
        if self.keys is None:
            n = self.snap.count
            hits, _ = self.eng.searchBatchHits(self.seq.queries, n)
            self.keys = np.empty((S.N_QUERIES, n), dtype=np.int64)
            for qi in range(S.N_QUERIES):
                keys = hits[qi, :, 0]
                keys = keys[keys != GR.KEY_PAD]
                assert len(keys) == n
                by_row = np.empty(n, dtype=np.int64)
                by_row[GR.key_rows(keys)] = keys
                finite = np.isfinite(GR.unorder_bits(GR.key_bits(by_row)))
                self.keys[qi] = np.where(finite, by_row, GR.KEY_PAD)
        return self.keys

    def grouped(self, qi, pred, limit, per_group, cut_at=None):
        """What searchGrouped must return (test_grouped_gpu.check): roots, score bits, member ids, member score bits, counts — the model on
        the fresh engine's row keys, which the fresh engine's own searchGrouped must equal too. cut_at: minScore = that group's score."""
        key = (qi, pred, limit, per_group, cut_at)
        if key not in self.grouped_cache:
            snap, metric = self.snap, METRIC_NAMES[self.seq.metric]
            if qi not in self.by_key:
                self.by_key[qi] = np.argsort(self.row_keys()[qi], kind="stable")
            if self.root_index is None:
                self.root_index = np.unique(GR.roots_of(snap.parent, snap.ids), return_inverse=True)
            ans = S.grouped_answer(self.row_keys()[qi], snap.parent, snap.ids, None if pred is None else snap.mask(pred), limit, per_group,
                                   self.by_key[qi], self.root_index)
            cut = None
            if cut_at is not None and len(ans.bits) > cut_at:
                cut = float(GR.score_of(ans.bits, metric)[cut_at])
                ans = GR.apply_cut(ans, cut, metric)
            filled = ans.member_keys != GR.KEY_PAD
            exp = (ans.roots, GR.score_of(ans.bits, metric).view(np.int32),
                   np.where(filled, snap.ids[GR.key_rows(ans.member_keys) % snap.count], GR.ID_PAD),
                   np.where(filled, GR.score_of(GR.key_bits(ans.member_keys), metric), np.float32(0.0)).astype(np.float32).view(np.int32), ans.counts)
            kw = S.PREDICATES[pred] if pred else {}
            own = self.eng.searchGrouped(self.seq.queries[qi], limit, per_group, minScore=cut, **kw)
            assert same_grouped(own, exp), f"the rebuilt store's own searchGrouped q{qi} pred {pred} ({limit}, {per_group}) cut {cut}"
            self.grouped_cache[key] = exp, cut
        return self.grouped_cache[key]

    def parity(self, qi, k, pred, listed, got, req=None):
        key = (qi, pred, listed, req)
        if key not in self.oracle_cache:
            rows = np.flatnonzero(self.mask(pred, listed, req))
            if len(rows) == 0:
                self.oracle_cache[key] = (np.zeros(0, dtype=np.uint64), np.zeros(0))
            else:
                ids, scores, _, _ = oracle.search(self.seq.metric, self.matrix[rows], self.snap.ids[rows], self.seq.queries[qi],
                                                  max(S.KS) + PARITY_MARGIN)
                self.oracle_cache[key] = (ids, scores)
        ids, scores = self.oracle_cache[key]
        assert_parity(got[0], got[1], ids[:k], scores[:k], all_exp_scores=scores, ctx=f"oracle parity q{qi} k{k} pred {pred} listed {listed} required {req}")


class Run:
    """One engine under test, one sequence."""

    def __init__(self, wax, name, sharded=False):
        self.wax, self.seq, self.sharded = wax, S.sequence(name), sharded
        seq = self.seq
        kw = {"devices": [0] * 3} if sharded else {}
        self.eng = wax.HIPVectorEngine(metric=wax.VectorMetric(seq.metric), dimensions=seq.dims, **kw)
        if sharded:
            self.eng.setTuning("shard_min_mb", 0)
        self.eng.setTuning("compact_window_rows", S.COMPACT_WINDOW)
        self.margins = S.margins(name) if seq.mirror and not sharded else None
        # the second, untouched engine of the searchMany readers
        self.other = wax.HIPVectorEngine(metric=wax.VectorMetric(seq.metric), dimensions=seq.dims)
        self.other_rows = seq.pool.rows[:300]
        self.other.addBatch(np.arange(300, dtype=np.uint64) + 5_000_000, self.other_rows)
        self.other.setTuning("scan_mirror", 0)
        self.other_ref = {}
        self.si, self.ref, self.ctx = 0, None, ""
        self.side = None
        if not sharded:                                                  # the stream of the timelineDevice reads
            import torch
            self.torch, self.dev = torch, torch.device("cuda", 0)
            self.side = torch.cuda.Stream(self.dev)

    def close(self):
        self.eng.close()
        self.other.close()

    # -- helpers
    def switches(self, **kw):
        for key, value in {**SWITCHES, **kw}.items():
            self.eng.setTuning(key, value)

    def get(self, *names):
        return {n: self.eng.getTuning(n) for n in names}

    def delta(self, before):
        return {n: self.eng.getTuning(n) - v for n, v in before.items()}

    def expect(self, got, qi, k, pred=None, listed=False, what="", req=None):
        ref = self.ref.answer(qi, k, pred, listed, req)
        assert same(got, ref), f"{self.ctx}: {what} q{qi} k{k} pred {pred} listed {listed} required {req}: {got} != {ref}"

    def certifies(self, bits, pred=None, queries=range(S.N_QUERIES), ks=S.KS):
        """Every listed (query, k) of this step is in the certifying class of that mirror (never on the handle or the l2 store)."""
        if self.margins is None:
            return False
        f = self.margins.margin8 if bits == 8 else self.margins.margin16
        return all(f(self.si, qi, k, pred) >= S.PM.MARGIN_FLOOR for qi in queries for k in ks)

    # -- the mutations
    def apply(self, op):
        eng, pool = self.eng, self.seq.pool
        kind = op[0]
        if kind == "addBatch":
            eng.addBatch(np.array(op[1], dtype=np.uint64), pool.rows[np.asarray(op[2], dtype=np.int64)])
        elif kind == "add":
            eng.add(int(op[1]), pool.rows[int(op[2])])
        elif kind == "remove":
            eng.remove(int(op[1]))
        elif kind == "removeBatch":
            eng.removeBatch(np.array(op[1], dtype=np.uint64))
        elif kind == "setAttributes":
            assert eng.setAttributes(np.array(op[1], dtype=np.uint64), op[2], op[3]) == len(op[1]), self.ctx
        elif kind == "setParents":
            eng.setParents(np.array(op[1], dtype=np.uint64), np.array(op[2], dtype=np.uint64))
        elif kind == "setTerms":
            eng.setTerms(np.array(op[1], dtype=np.uint64), op[2])
        elif kind == "reserve":
            eng.reserve(int(op[1]))
        elif kind == "roundtrip":
            eng.deserialize(eng.serialize())
        elif kind == "deserialize_blob":
            eng.deserialize(S.blob_of(self.seq, op[1], op[2]))
        else:
            raise AssertionError(kind)

    # -- the readers
    def read_f32(self):
        self.switches()
        c = self.get("mirror_scans")
        for qi in range(S.N_QUERIES):
            for k in S.KS:
                self.expect(self.eng.searchArrays(self.seq.queries[qi], k), qi, k, what="f32 scan")
        assert self.delta(c)["mirror_scans"] == 0

    def read_bf16_alone(self):
        self.switches(scan_mirror=2)
        c = self.get("mirror_scans", "mirror8_passes", "mirror_scan_fallbacks")
        for qi in range(S.N_QUERIES):
            for k in S.KS:
                self.expect(self.eng.searchArrays(self.seq.queries[qi], k), qi, k, what="bf16 pass, alone")
        d = self.delta(c)
        if self.seq.mirror:
            if not self.sharded:
                assert (d["mirror_scans"], d["mirror8_passes"]) == (len(S.KS) * S.N_QUERIES, 0), (self.ctx, d)
            if self.certifies(16):
                assert d["mirror_scan_fallbacks"] == 0, (self.ctx, d)
        else:
            assert d["mirror_scans"] == 0, (self.ctx, d)               # no mirror kernel at this dimension: the f32 scan answered

    def tickets(self, k, preds):
        eng, qs = self.eng, self.seq.queries
        ts = [eng.submit(qs[qi], k) if p is None else eng.submitFiltered(qs[qi], k, **S.PREDICATES[p]) for qi, p in enumerate(preds)]
        return [eng.collect(t, k) for t in ts]

    def read_bf16_parked(self):
        self.switches(scan_mirror=2, mirror_share=2)
        c = self.get("mirror_shared_passes", "mirror8_passes", "mirror_scan_fallbacks")
        for k in S.KS:
            for qi, got in enumerate(self.tickets(k, [None] * S.N_QUERIES)):
                self.expect(got, qi, k, what="bf16 pass, four parked tickets")
        d = self.delta(c)
        if self.seq.mirror and not self.sharded:
            assert (d["mirror_shared_passes"], d["mirror8_passes"]) == (len(S.KS), 0), (self.ctx, d)
            if self.certifies(16):
                assert d["mirror_scan_fallbacks"] == 0, (self.ctx, d)

    def read_code8_alone(self):
        self.switches(scan_mirror=2, mirror_bits=8)
        c = self.get("mirror8_fallbacks", "mirror_scan_fallbacks")
        for _ in range(3):                                               # a stale code mirror: two on bf16, the third rebuilds it
            self.expect(self.eng.searchArrays(self.seq.queries[0], 10), 0, 10, what="8-bit pass, warm-up")
        p = self.get("mirror8_passes")
        for qi in range(S.N_QUERIES):
            for k in S.KS:
                self.expect(self.eng.searchArrays(self.seq.queries[qi], k), qi, k, what="8-bit pass, alone")
        if self.seq.mirror and not self.sharded:
            assert self.delta(p)["mirror8_passes"] == len(S.KS) * S.N_QUERIES, self.ctx
            if self.certifies(8) and self.certifies(16, queries=[0], ks=[10]):
                assert set(self.delta(c).values()) == {0}, (self.ctx, self.delta(c))
        elif not self.seq.mirror:
            assert self.delta(p)["mirror8_passes"] == 0, self.ctx

    def read_code8_tickets(self):
        """Two unfiltered and two submitFiltered tickets of predicate A in one parked set."""
        self.switches(scan_mirror=2, mirror_bits=8, mirror_share=2, predicate_mirror=2)
        preds = [None, None, "A", "A"]
        c = self.get("mirror8_fallbacks", "mirror_scan_fallbacks", "predicate_mirror_fallbacks")
        before = self.eng.predicateTicketStats()
        for k in S.KS:
            for qi, got in enumerate(self.tickets(k, preds)):
                self.expect(got, qi, k, pred=preds[qi], what="8-bit pass, four tickets")
        after = self.eng.predicateTicketStats()
        assert after["submitted"] - before["submitted"] == 2 * len(S.KS), self.ctx
        if self.certifies(8) and self.certifies(16) and self.certifies(8, "A", [2, 3]) and self.certifies(16, "A", [2, 3]):
            assert after["fallbacks"] == before["fallbacks"] and set(self.delta(c).values()) == {0}, (self.ctx, after, self.delta(c))

    def read_batch(self):
        self.switches()
        qs = self.seq.batch_queries
        for k in S.KS:
            ids, scores, counts = self.eng.searchBatch(qs, k)
            for qi in range(S.N_BATCH):
                ref = self.ref.answer(qi, k)
                assert same((ids[qi][:counts[qi]], scores[qi][:counts[qi]]), ref), f"{self.ctx}: searchBatch q{qi} k{k}"

    def read_allow_lists(self):
        for dev_min, what in ((0, "device table"), (-1, "host probe")):
            self.switches(filter_device_min=dev_min)
            c = self.get("filter_device_searches")
            for qi in range(S.N_QUERIES):
                for k in S.KS:
                    self.expect(self.eng.searchFiltered(self.seq.queries[qi], k, frameIds=self.ref.allow), qi, k, listed=True, what="allow-list, " + what)
            if not self.sharded:
                assert self.delta(c)["filter_device_searches"] == (len(S.KS) * S.N_QUERIES if dev_min == 0 else 0), self.ctx

    def read_predicates(self):
        names = ("predicate_gather_searches", "predicate_masked_scans", "predicate_mirror_scans", "predicate_mirror_fallbacks")
        for route in (1, 2):
            for pred in ("A", "B"):
                self.switches(predicate_route=route, predicate_mirror=2)
                c = self.get(*names)
                for qi in range(S.N_QUERIES):
                    for k in S.KS:
                        got = self.eng.searchFiltered(self.seq.queries[qi], k, **S.PREDICATES[pred])
                        self.expect(got, qi, k, pred=pred, what=f"predicate, route {route}")
                d = self.delta(c)
                m = int(self.ref.snap.mask(pred).sum())
                if self.sharded:
                    continue
                n = len(S.KS) * S.N_QUERIES
                if m == 0:
                    assert set(d.values()) == {0}, (self.ctx, d)
                elif route == 1 or not self.seq.mirror:
                    assert (d["predicate_gather_searches"], d["predicate_masked_scans"]) == (n, 0), (self.ctx, route, pred, d)   # (100 dimensions: no masked scan)
                else:
                    assert (d["predicate_gather_searches"], d["predicate_masked_scans"]) == (0, n), (self.ctx, pred, d)
                    if m > S.KP:
                        assert d["predicate_mirror_scans"] + d["predicate_mirror_fallbacks"] == n, (self.ctx, pred, d)
                        if self.certifies(16, pred):
                            assert d["predicate_mirror_fallbacks"] == 0, (self.ctx, pred, d)

    def read_batch_filtered(self):
        """Lists and predicates per query: q0 list + A, q1 A, q2 list, q3 B."""
        self.switches(filter_device_min=0)
        allow = self.ref.allow
        plan = [("A", True), ("A", False), (None, True), ("B", False)]
        for k in S.KS:
            ids, scores, counts = self.eng.searchBatchFiltered(
                self.seq.queries, k, frameIds=[allow, None, allow, None],
                timeRange=[None, None, None, S.PRED_B["timeRange"]], denyFlags=[1, 1, 0, 0])
            for qi, (pred, listed) in enumerate(plan):
                self.expect((ids[qi][:counts[qi]], scores[qi][:counts[qi]]), qi, k, pred=pred, listed=listed, what="searchBatchFiltered")

    def read_many(self):
        if self.sharded:
            return                                                       # wax_hip_search_many refuses a handle
        self.switches()
        wax, qs = self.wax, self.seq.queries
        engines = [self.eng, self.other, self.eng, self.other]
        for k in S.KS:
            for filtered in (False, True):
                if filtered:
                    ids, scores, counts = wax.searchManyFiltered(engines, qs, k, denyFlags=1)
                else:
                    ids, scores, counts = wax.searchMany(engines, qs, k)
                for i in range(4):
                    got = (ids[i][:counts[i]], scores[i][:counts[i]])
                    if engines[i] is self.eng:
                        self.expect(got, i, k, pred="A" if filtered else None, what="searchMany")
                    else:                                                # the untouched store has no attributes: every row passes
                        if (i, k) not in self.other_ref:
                            self.other_ref[(i, k)] = self.other.searchArrays(qs[i], k)
                        assert same(got, self.other_ref[(i, k)]), f"{self.ctx}: searchMany, the untouched engine, pair {i}"

    def read_timeline(self):
        """Both orders x None, A, B x limits 10, 300 (and 1 without a predicate) and one limit-4096 list per order, which pairs (nearly)
        every id with its timestamp: a column that missed a shift shows even where no top row moved. A frame id two rows hold appears
        twice."""
        eng, seq, snap = self.eng, self.seq, self.ref.snap
        device = []
        for newest in (True, False):
            for pred in (None, "A", "B"):
                kw = S.PREDICATES[pred] if pred else {}
                limits = ((1,) if pred is None else ()) + (10, 300) + ((TL.MAX_LIMIT,) if pred == S.LONG_TIMELINE[newest] else ())
                whole = seq.timeline(snap, limits[-1], newest, pred)         # (the model's answer to a limit is a prefix of its answer to a larger one)
                for limit in limits:
                    exp = whole[0][:limit], whole[1][:limit]
                    got = eng.timeline(limit, newestFirst=newest, **kw)
                    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]), f"{self.ctx}: timeline newest {newest} pred {pred} limit {limit}"
                    if self.side is not None and limit == limits[-1]:      # (the device form once per order and predicate, at its largest limit)
                        d_ids = self.torch.zeros(limit, dtype=self.torch.int64, device=self.dev)
                        d_cnt = self.torch.full((1,), 99, dtype=self.torch.int32, device=self.dev)
                        eng.timelineDevice(limit, d_ids, d_cnt, newestFirst=newest, stream=self.side.cuda_stream, **kw)
                        device.append((d_ids, d_cnt, exp[0], limit, (newest, pred)))
        if self.side is not None:
            self.side.synchronize()
            for d_ids, d_cnt, ids, limit, what in device:
                assert int(d_cnt.cpu()[0]) == len(ids), f"{self.ctx}: timelineDevice count {what} limit {limit}"
                assert np.array_equal(d_ids.cpu().numpy().view(np.uint64), TL.padded(ids, limit)), f"{self.ctx}: timelineDevice {what} limit {limit}"

    def read_grouped(self):
        """One checked query per step, each in its turn, at (limit 10, perGroup 3) under None, A and B; query 0 at (1024, 8) and (1, 1), one
        minScore cut at the fifth group's score; one query under "force_general" where the fused scan serves the dimension. (A handle:
        one member per group.)"""
        eng, seq = self.eng, self.seq
        self.switches()
        members = (lambda p: 1) if self.sharded else (lambda p: p)
        turn = (self.si + 1) % S.N_QUERIES                             # the query whose two best rows the step's planted setParents names
        plan = [(turn, pred, 10, members(3), None) for pred in (None, "A", "B")]
        plan += [(0, None, GR.MAX_LIMIT, members(8), None), (0, None, 1, 1, None), (0, None, 10, members(3), 4)]
        before = eng.groupStats()
        # without attribute columns a predicate is decided on the host: A passes every row, B none — and that search is not counted
        counted = lambda pred: 0 if pred == "B" and not seq.steps[self.si].attr_column else 1

        def ask(qi, pred, limit, per_group, cut_at, what):
            exp, cut = self.ref.grouped(qi, pred, limit, per_group, cut_at)
            got = eng.searchGrouped(seq.queries[qi], limit, per_group, minScore=cut, **(S.PREDICATES[pred] if pred else {}))
            assert same_grouped(got, exp), f"{self.ctx}: searchGrouped, {what}, q{qi} pred {pred} ({limit}, {per_group}) cut {cut}: {got} != {exp}"

        for case in plan:
            ask(*case, what="fused scan" if seq.mirror else "column route")
        forced = 0
        if seq.mirror:
            eng.setTuning("force_general", 1)
            try:
                ask(turn, (None, "A", "B")[self.si % 3], 10, members(3), None, what="column route")
                forced = counted((None, "A", "B")[self.si % 3])
            finally:
                eng.setTuning("force_general", 0)
        if not self.sharded:
            d = {n: v - before[n] for n, v in eng.groupStats().items()}
            n = sum(counted(case[1]) for case in plan)
            fused, column = (n, forced) if seq.mirror else (0, n)                     # (100 dimensions: no fused scan)
            assert (d["searches"], d["fused_scans"], d["column_scans"]) == (n + forced, fused, column), (self.ctx, d)

    def read_terms(self):
        """R1 and R2, alone and with predicate A, on the three routes: one checked query per pair and step, each in its turn, at 10 results
        (and at 1 for R1 alone); R1 with the long allow-list on the device (the probe, then the AND) and with a short list staged on the
        host. Counter deltas per call."""
        eng, seq, snap = self.eng, self.seq, self.ref.snap
        column = seq.steps[self.si].term_column                          # else: no frame has metadata, the search is decided on the host

        def ask(qi, k, req, pred, listed, frame_ids, route, mirror, what):
            c, t = self.get(*PREDICATE_COUNTERS), eng.termStats()
            got = eng.searchFiltered(seq.queries[qi], k, frameIds=frame_ids, requiredTerms=list(req), **(S.PREDICATES[pred] if pred else {}))
            self.expect(got, qi, k, pred=pred, listed=listed, req=req, what=what)
            if self.sharded:
                return
            d, t1 = self.delta(c), eng.termStats()
            dt = {n: t1[n] - t[n] for n in ("searches", "device_masks", "host_staged", "host_decided")}
            m = int(self.ref.mask(pred, listed, req).sum())
            if not column:
                assert len(got[0]) == 0 and m == 0, (self.ctx, what)
                assert dt == {"searches": 1, "device_masks": 0, "host_staged": 0, "host_decided": 1} and set(d.values()) == {0}, (self.ctx, what, dt, d)
                return
            staged = listed == "short"
            assert dt == {"searches": 1, "device_masks": 0 if staged else 1, "host_staged": 1 if staged else 0, "host_decided": 0}, (self.ctx, what, dt)
            fell = d.pop("predicate_mirror_fallbacks")
            if m == 0:
                assert set(d.values()) == {0} and fell == 0, (self.ctx, what, d)
            elif staged or route == 1 or not seq.mirror:                 # (100 dimensions: no masked scan)
                assert (d["predicate_gather_searches"], d["predicate_masked_scans"], d["predicate_mirror_scans"], fell) == (1, 0, 0, 0), (self.ctx, what, d)
            elif route == 2:
                assert (d["predicate_gather_searches"], d["predicate_masked_scans"]) == (0, 1), (self.ctx, what, d)
                assert d["predicate_mirror_scans"] + fell == (1 if mirror == 2 and m > S.KP else 0), (self.ctx, what, d, fell, m)
                if mirror == 2 and self.margins.margin16(self.si, qi, k, pred, req) >= S.PM.MARGIN_FLOOR:
                    assert fell == 0, (self.ctx, what, d)

        for route, mirror in TERM_ROUTES:
            self.switches(predicate_route=route, predicate_mirror=mirror)
            for turn, (req, pred) in enumerate(((S.R1, None), (S.R1, "A"), (S.R2, None), (S.R2, "A"))):
                qi = (self.si + turn) % S.N_QUERIES                      # ((R1, None) asks the query whose top row the step's planted setTerms names)
                if route != 1 and turn and not seq.mirror:
                    continue                                             # (100 dimensions: every route gathers; the other two ask R1 alone)
                for k in S.KS if turn == 0 else S.KS[-1:]:
                    ask(qi, k, req, pred, False, None, route, mirror, f"required terms, route {route} mirror {mirror}")
        qi = self.si % S.N_QUERIES
        self.switches(filter_device_min=0)
        ask(qi, 10, S.R1, None, True, self.ref.allow, 0, 0, "required terms and the long allow-list")
        self.switches()
        ask(qi, 10, S.R1, None, "short", self.ref.short, 0, 0, "required terms and a short allow-list")

    READERS = ("read_f32", "read_bf16_alone", "read_bf16_parked", "read_code8_alone", "read_code8_tickets", "read_batch",
               "read_allow_lists", "read_predicates", "read_batch_filtered", "read_many", "read_timeline", "read_grouped", "read_terms")

    # -- the store itself
    def check_store(self):
        eng, snap, seq = self.eng, self.ref.snap, self.seq
        assert eng.count == snap.count, self.ctx
        assert eng.serialize() == oracle.mv2v_serialize(seq.metric, self.ref.matrix, snap.ids), f"{self.ctx}: serialize"
        uniq, first = np.unique(snap.ids, return_index=True)
        ts, fl, found = eng.getAttributes(np.concatenate([uniq, np.array([S.ABSENT_ID], dtype=np.uint64)]))
        assert found[:-1].all() and not found[-1] and ts[-1] == 0 and fl[-1] == 0, f"{self.ctx}: getAttributes found"
        assert np.array_equal(ts[:-1], snap.ts[first]) and np.array_equal(fl[:-1], snap.fl[first]), f"{self.ctx}: getAttributes"
        par, found = eng.getParents(np.concatenate([uniq, np.array([S.ABSENT_ID], dtype=np.uint64)]))
        assert found[:-1].all() and not found[-1] and par[-1] == GR.NO_PARENT, f"{self.ctx}: getParents found"
        assert np.array_equal(par[:-1], snap.parent[first]), f"{self.ctx}: getParents"
        # getTerms: the ids the step's column ops named, the shared id, a seeded sample of 64, one absent id
        named = set()
        for op in seq.steps[self.si].ops:
            if op[0] in S.COLUMN_OPS:                                    # (of an op that names the whole store: every 16th id and the last ones)
                named |= {int(i) for i in (op[1] if len(op[1]) <= 256 else list(op[1][::16]) + list(op[1][-4:]))}
        sample = np.random.default_rng(self.si).choice(uniq, min(64, len(uniq)), replace=False)
        row_of = dict(zip(uniq.tolist(), first.tolist()))
        for fid in named | {S.shared_id(seq.name)} | {int(i) for i in sample}:
            got = eng.getTerms(fid)
            if fid in row_of:
                assert got is not None and tuple(got.tolist()) == snap.terms[row_of[fid]], f"{self.ctx}: getTerms {fid}: {got} != {snap.terms[row_of[fid]]}"
            else:
                assert got is None, f"{self.ctx}: getTerms of a frame not held {fid}"
        assert eng.getTerms(S.ABSENT_ID) is None, f"{self.ctx}: getTerms of an absent id"

    def run(self):
        t0 = time.perf_counter()
        for si, step in enumerate(self.seq.steps):
            self.si, self.ctx = si, f"{self.seq.name}{' x3' if self.sharded else ''} step {si} ({step.name})"
            before = self.get(*STEP_COUNTERS)
            columns = None if self.sharded else {**self.eng.groupStats(), **self.eng.termStats()}
            for op in step.ops:
                self.apply(op)
            self.ref = Reference(self.wax, self.seq, step.after)
            try:
                order = self.READERS[si % len(self.READERS):] + self.READERS[:si % len(self.READERS)]
                for name in order:
                    getattr(self, name)()
                self.check_store()
                if not self.sharded:
                    assert self.delta(before) == step.counters, f"{self.ctx}: counters {self.delta(before)}, predicted {step.counters}; first reader {order[0]}"
                    now = {**self.eng.groupStats(), **self.eng.termStats()}
                    got = {n: now[n] - (0 if n == "group_slots" else columns[n]) for n in S.COLUMN_COUNTERS}      # ("group_slots" is what the last grouped search saw)
                    assert got == step.column_counters, f"{self.ctx}: column counters {got}, predicted {step.column_counters}; first reader {order[0]}"
            finally:
                self.ref.close()
        print(f"\n[{self.ctx.split(' step')[0]}] {len(self.seq.steps)} steps in {time.perf_counter() - t0:.2f} s")


def run(wax, name, sharded=False):
    r = Run(wax, name, sharded)
    try:
        r.run()
    finally:
        r.close()


def test_cosine_5003_x_384(wax):
    run(wax, "cos384")


def test_dot_2101_x_768(wax):
    run(wax, "dot768")


def test_l2_700_x_100_growing_past_2048(wax):
    run(wax, "l2_100")


def test_cosine_on_a_handle_of_three_shards(wax):
    run(wax, "cos384", sharded=True)
