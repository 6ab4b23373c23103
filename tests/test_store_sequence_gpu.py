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

What the sequence found (fixed in this commit): after `deserialize` of a segment in which two rows hold one frame id, `remove` of that
id took the lower row and dropped the id from the host map, so the surviving row could no longer be addressed: a second `remove` was a
no-op, an upsert appended a third row, `getAttributes` reported the frame missing and the host probe of an allow-list disagreed with
the device table. Exposed by the step "upsert of the shared id" (count and serialize) and, one step earlier, by getAttributes."""
import time

import numpy as np
import pytest

import oracle
import store_sequence_ref as S
from helpers import assert_parity

pytestmark = pytest.mark.gpu

PARITY_MARGIN = 8
STEP_COUNTERS = ("mirror_rows_converted", "idhash_rows_inserted", "mirror8_conversions", "mirror8_rows_converted")
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
        self.eng.setTuning("scan_mirror", 0)
        self.eng.setTuning("filter_device_min", -1)
        self.allow = np.array([i for i in snap.ids if allowed(i)] + [S.ABSENT_ID], dtype=np.uint64)
        self.in_allow = np.isin(snap.ids, self.allow)
        self.cache, self.oracle_cache = {}, {}

    def close(self):
        self.eng.close()

    def mask(self, pred, listed):
        m = self.snap.mask(pred)
        return m & self.in_allow if listed else m

    def answer(self, qi, k, pred=None, listed=False):
        """qi indexes the 32 batch queries; the first four are the checked ones (the only ones asked with a filter, and held to the oracle)."""
        key = (qi, k, pred, listed)
        if key not in self.cache:
            q = self.seq.batch_queries[qi]
            if pred is None and not listed:
                got = self.eng.searchArrays(q, k)
            else:
                got = self.eng.searchFiltered(q, k, frameIds=self.snap.ids[self.mask(pred, listed)])
            self.cache[key] = got
            if qi < S.N_QUERIES:
                self.parity(qi, k, pred, listed, got)
        return self.cache[key]

    def parity(self, qi, k, pred, listed, got):
        key = (qi, pred, listed)
        if key not in self.oracle_cache:
            rows = np.flatnonzero(self.mask(pred, listed))
            if len(rows) == 0:
                self.oracle_cache[key] = (np.zeros(0, dtype=np.uint64), np.zeros(0))
            else:
                ids, scores, _, _ = oracle.search(self.seq.metric, self.matrix[rows], self.snap.ids[rows], self.seq.queries[qi],
                                                  max(S.KS) + PARITY_MARGIN)
                self.oracle_cache[key] = (ids, scores)
        ids, scores = self.oracle_cache[key]
        assert_parity(got[0], got[1], ids[:k], scores[:k], all_exp_scores=scores, ctx=f"oracle parity q{qi} k{k} pred {pred} listed {listed}")


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

    def expect(self, got, qi, k, pred=None, listed=False, what=""):
        ref = self.ref.answer(qi, k, pred, listed)
        assert same(got, ref), f"{self.ctx}: {what} q{qi} k{k} pred {pred} listed {listed}: {got} != {ref}"

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

    READERS = ("read_f32", "read_bf16_alone", "read_bf16_parked", "read_code8_alone", "read_code8_tickets", "read_batch",
               "read_allow_lists", "read_predicates", "read_batch_filtered", "read_many")

    # -- the store itself
    def check_store(self):
        eng, snap, seq = self.eng, self.ref.snap, self.seq
        assert eng.count == snap.count, self.ctx
        assert eng.serialize() == oracle.mv2v_serialize(seq.metric, self.ref.matrix, snap.ids), f"{self.ctx}: serialize"
        uniq, first = np.unique(snap.ids, return_index=True)
        ts, fl, found = eng.getAttributes(np.concatenate([uniq, np.array([S.ABSENT_ID], dtype=np.uint64)]))
        assert found[:-1].all() and not found[-1] and ts[-1] == 0 and fl[-1] == 0, f"{self.ctx}: getAttributes found"
        assert np.array_equal(ts[:-1], snap.ts[first]) and np.array_equal(fl[:-1], snap.fl[first]), f"{self.ctx}: getAttributes"

    def run(self):
        t0 = time.perf_counter()
        for si, step in enumerate(self.seq.steps):
            self.si, self.ctx = si, f"{self.seq.name}{' x3' if self.sharded else ''} step {si} ({step.name})"
            before = self.get(*STEP_COUNTERS)
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
