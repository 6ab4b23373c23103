"""The three passes that scan under a row bitmap in a persistent grid — code8_pass<MASKED> (the predicate tickets' pass over the 8-bit
code mirror), mirror_pass<MASKED> (the bf16 mirror form of a predicate search) and scan_masked_kernel (the f32 store) — with every
wave running MANY iterations: each fetches the bitmap word of its next chunk an iteration ahead, takes this chunk's bits from the word
fetched before, and leaves a chunk without a passing row at once. Elsewhere in the suite the two mirror passes give every wave one
chunk whenever the bitmap is not all ones, and the f32 scan at most four (the small-store rule of its grid on 20 005 rows).

Stores of 4 099 rows (384-d and 768-d, cosine and dot) under "grid_blocks" 1, 2 and 3 — 22 to 129 iterations per wave, 513 in the f32
scan at 768-d, a ragged last one at 3 workgroups — and masks built on the iteration that owns a row (masked_iterations_ref.py), so
that the word of a neighbouring iteration is the wrong one everywhere; and one store of 65 553 rows at the default grid (342
workgroups, three iterations). Every masked answer is held to two references that share no loop with the pass under test:
  (a) searchFiltered(q, k, frameIds = the passing ids) on the same engine, ids and scores array_equal: an allow-list without a
      predicate is gathered and scored row by row, no bitmap is read in a scan loop (the masked counters are shown not to move);
  (b) the oracle's f64 ranking of the passing rows, under helpers.assert_parity.
The counters say that the pass under test answered: a fallback would let a broken pass hide behind the f32 scan, so none is allowed,
and tests/test_masked_iterations_cpu.py shows first that every case sent here certifies in the float64 models of both certificates."""
import numpy as np
import pytest

import masked_iterations_ref as I
import oracle
from helpers import assert_parity

pytestmark = pytest.mark.gpu

COUNTERS = ("predicate_searches", "predicate_gather_searches", "predicate_masked_scans", "predicate_mirror_scans",
            "predicate_mirror_fallbacks", "predicate_mirror_unavailable")
PER_QUERY = {"f32": [1, 0, 1, 0, 0, 0], "bf16": [1, 0, 1, 1, 0, 0]}
TUNING = {"f32": (("predicate_route", 2), ("predicate_mirror", 0)),
          "bf16": (("predicate_route", 2), ("predicate_mirror", 2), ("mirror_bits", 16)),
          "code8": (("predicate_mirror", 2), ("mirror_bits", 8), ("scan_mirror", 2), ("mirror_share", 2))}
STAT_KEYS = ("submitted", "rode", "masked_passes", "certified", "fallbacks", "deferred")
SET_SIZES = (1, 2, 3, 4)
ORACLE_MARGIN = 10


@pytest.fixture(scope="module")
def wax(hip_lib):
    import wax_amd
    if hip_lib.wax_hip_device_count() == 0:
        pytest.skip("no HIP device on this host: the gpu-marked tests run on the MI355X box (pytest -m gpu)")
    assert hip_lib.wax_hip_available() == 1, "a HIP device is visible but it is not gfx950: the HIP path needs an MI355X"
    return wax_amd


class Store:
    """An engine over a store of masked_iterations_ref.py, tuned to one form, with ts = row and the masks in the flag column (a row
    fails a mask iff the mask's bit is set); the references of every (mask, query, top_k) it is asked for."""

    def __init__(self, wax, name, form):
        self.name, self.form = name, form
        self.metric, self.n, self.dims = I.shape_of(name)
        self.rows, self.queries = I.store_rows(name), I.queries_of(name)
        self.ids = np.arange(self.n, dtype=np.uint64) * 3 + 7
        self.ts = np.arange(self.n, dtype=np.int64)
        self.eng = wax.HIPVectorEngine(metric=wax.VectorMetric(self.metric), dimensions=self.dims)
        self.eng.addBatch(self.ids, self.rows)
        for key, value in TUNING[form]:
            self.eng.setTuning(key, value)
        self.masks, self.best, self.refs = {}, {}, {}

    def set_grid(self, grid_blocks, mask_names=I.MASKS):
        """"grid_blocks", and the masks of this form's (C, W) under it into the flag column."""
        self.eng.setTuning("grid_blocks", grid_blocks)
        c, w = I.waves_of(self.form, self.n, self.dims, grid_blocks)
        all_masks = I.masks(self.n, self.dims, c, w)
        self.masks = {m: all_masks[m] for m in mask_names}
        self.best, self.refs = {}, {}
        fl = I.flags_for(self.masks)
        assert self.eng.setAttributes(self.ids, self.ts, fl) == self.n
        for m, mask in self.masks.items():
            assert np.array_equal((fl & np.uint32(I.MASK_BIT[m])) == 0, mask)
        if self.form == "code8":                      # a stale or missing code mirror is rebuilt by the third query in a row that wants it
            for _ in range(3):
                self.eng.searchArrays(self.queries[0], 1)
        return c, w

    def counters(self):
        return [self.eng.getTuning(c) for c in COUNTERS]

    def stats(self):
        st = self.eng.predicateTicketStats()
        return {k: st[k] for k in STAT_KEYS}

    def reference(self, m, q, k):
        """(a): the allow-list of the passing ids, on this engine; computed once per (mask, query, top_k)."""
        if (m, q, k) not in self.refs:
            before, passes = self.counters(), self.stats()["masked_passes"]
            self.refs[m, q, k] = self.eng.searchFiltered(self.queries[q], k, frameIds=self.ids[self.masks[m]])
            assert self.counters() == before and self.stats()["masked_passes"] == passes, "the reference took a masked pass"
        return self.refs[m, q, k]

    def check(self, got, m, q, k, ctx):
        """One masked answer against (a) and (b)."""
        ref = self.reference(m, q, k)
        assert np.array_equal(got[0], ref[0]), f"{ctx}: ids {got[0]} differ from the allow-list reference {ref[0]}"
        assert np.array_equal(got[1], ref[1]), f"{ctx}: scores differ from the allow-list reference"
        passing = np.flatnonzero(self.masks[m])
        assert len(got[0]) == min(k, len(passing)), ctx
        if (m, q) not in self.best:                   # the oracle's ranking of the passing rows, as far as any top_k here needs it
            deepest = min(max(I.KS[self.form]) + ORACLE_MARGIN, len(passing))
            self.best[m, q] = oracle.search(self.metric, self.rows[passing], self.ids[passing], self.queries[q], deepest)[:2]
        ei, es = self.best[m, q]
        assert_parity(got[0], got[1], ei[:k], es[:k], all_exp_scores=es[:k + ORACLE_MARGIN], ctx=ctx)


def run_blocking(s, mask_names, ks, ctx):
    """searchFiltered under every mask and top_k, every query: the answers, and the counters of the form per query."""
    nq = len(s.queries)
    for m in mask_names:
        deny = I.MASK_BIT[m]
        for k in ks:
            for q in range(nq):
                s.reference(m, q, k)
            before = s.counters()
            got = [s.eng.searchFiltered(s.queries[q], k, denyFlags=deny) for q in range(nq)]
            delta = [a - b for a, b in zip(s.counters(), before)]
            for q in range(nq):
                s.check(got[q], m, q, k, f"{ctx} {m} top_k {k} query {q}")
            assert delta == [nq * x for x in PER_QUERY[s.form]], f"{ctx} {m} top_k {k}: counters {dict(zip(COUNTERS, delta))}"


def run_set(s, members, k, ctx, free=None):
    """Park the members — (query, mask; None = an unfiltered ticket) — and collect them in order: one set of "mirror_share" 2, one
    masked pass. Every masked member rode, was certified and equals its references; the unfiltered one equals the exact scan."""
    assert 1 <= len(members) <= 4
    for q, m in members:
        if m is not None:
            s.reference(m, q, k)
    masked = sum(1 for _, m in members if m is not None)
    before, fallbacks8 = s.stats(), s.eng.getTuning("mirror8_fallbacks")
    tickets = [s.eng.submit(s.queries[q], k) if m is None else s.eng.submitFiltered(s.queries[q], k, denyFlags=I.MASK_BIT[m]) for q, m in members]
    got = [s.eng.collect(t, k) for t in tickets]
    now = s.stats()
    d = {key: now[key] - before[key] for key in STAT_KEYS}
    for (q, m), hits in zip(members, got):
        if m is None:
            assert np.array_equal(hits[0], free[q, k][0]) and np.array_equal(hits[1], free[q, k][1]), f"{ctx}: the unfiltered member differs from the exact scan"
        else:
            s.check(hits, m, q, k, f"{ctx} member ({q}, {m})")
    want = {"submitted": masked, "rode": masked, "masked_passes": 1, "certified": masked, "fallbacks": 0, "deferred": 0}
    assert d == want, f"{ctx}: {d}"
    assert s.eng.getTuning("mirror8_fallbacks") == fallbacks8, f"{ctx}: the unfiltered member was not certified"


def run_tickets(s, mask_names, ks, ctx, mixed_sets, set_sizes=SET_SIZES):
    nq = len(s.queries)
    for m in mask_names:                              # sets of one mask
        for k in ks:
            q0 = 0
            for size in set_sizes:
                run_set(s, [((q0 + i) % nq, m) for i in range(size)], k, f"{ctx} {m} top_k {k} set of {size}")
                q0 += size
    s.eng.setTuning("scan_mirror", 0)                 # the exact scan, for the unfiltered members
    free = {(q, k): s.eng.searchArrays(s.queries[q], k) for members in mixed_sets for q, m in members if m is None for k in ks}
    s.eng.setTuning("scan_mirror", 2)
    for members in mixed_sets:
        for k in ks:
            run_set(s, members, k, f"{ctx} {members} top_k {k}", free)
    assert s.eng.getTuning("mirror8_breaker_trips") == 0


# ---- 4 099 rows under "grid_blocks" 1, 2, 3 ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(I.STORES))
def test_f32_masked_scan_over_many_iterations(wax, name):
    s = Store(wax, name, "f32")
    try:
        for g in I.GRID_BLOCKS:
            c, w = s.set_grid(g)
            assert s.eng.getTuning("scan_grid") == g
            run_blocking(s, I.MASKS, I.KS["f32"], f"{name} f32, {g} workgroups ({I.iterations(s.n, c, w)[0]} iterations)")
    finally:
        s.eng.close()


@pytest.mark.parametrize("name", list(I.STORES))
def test_bf16_masked_pass_over_many_iterations(wax, name):
    s = Store(wax, name, "bf16")
    try:
        for g in I.GRID_BLOCKS:
            c, w = s.set_grid(g)
            run_blocking(s, I.MASKS, I.KS["bf16"], f"{name} bf16, {g} workgroups ({I.iterations(s.n, c, w)[0]} iterations)")
        assert s.eng.getTuning("predicate_mirror_fallbacks") == 0 and s.eng.getTuning("predicate_mirror_unavailable") == 0
    finally:
        s.eng.close()


@pytest.mark.parametrize("name", list(I.STORES))
def test_code8_masked_tickets_over_many_iterations(wax, name):
    s = Store(wax, name, "code8")
    try:
        for g in I.GRID_BLOCKS:
            c, w = s.set_grid(g)
            run_tickets(s, I.MASKS, I.KS["code8"], f"{name} 8 bits, {g} workgroups ({I.iterations(s.n, c, w)[0]} iterations)", I.MIXED_SETS)
        assert s.eng.getTuning("mirror8_breaker_trips") == 0 and s.eng.getTuning("mirror8_unavailable") == 0
    finally:
        s.eng.close()


# ---- 65 553 rows at the default grid: 342 workgroups, three iterations ---------------------------------------------------------------

def test_bf16_masked_pass_at_the_default_grid(wax):
    s = Store(wax, I.BIG, "bf16")
    try:
        assert s.set_grid(0, I.BIG_MASKS) == (16, 1368)
        run_blocking(s, I.BIG_MASKS, (10, 32), f"{I.BIG} bf16, default grid")
        assert s.eng.getTuning("predicate_mirror_fallbacks") == 0 and s.eng.getTuning("predicate_mirror_unavailable") == 0
    finally:
        s.eng.close()


def test_code8_masked_tickets_at_the_default_grid(wax):
    s = Store(wax, I.BIG, "code8")
    try:
        assert s.set_grid(0, I.BIG_MASKS) == (16, 1368)
        run_tickets(s, I.BIG_MASKS, (10, 16), f"{I.BIG} 8 bits, default grid", I.BIG_MIXED_SETS, set_sizes=(1, 4))
        assert s.eng.getTuning("mirror8_breaker_trips") == 0 and s.eng.getTuning("mirror8_unavailable") == 0
    finally:
        s.eng.close()
