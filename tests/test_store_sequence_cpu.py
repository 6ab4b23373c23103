"""What tests/test_store_sequence_gpu.py relies on, proved without a GPU on the sequences of store_sequence_ref.py: every step changes
an answer (so a structure that missed it answers visibly wrong), every coverage class is entered, at least nine in ten checked mirror
answers lie in the certifying class (margin >= predicate_mirror_ref.MARGIN_FLOOR: there the GPU test asserts zero fallbacks), the
model resolves a frame id that two rows hold to the lower row, and the counter predictions restate the rules the scripted tests
assert."""
import numpy as np
import pytest

import mirror8_planes_ref as P8
import mirror8_ref as R8
import oracle
import predicate_mirror_ref as PM
import store_sequence_ref as S
from helpers import OracleEngine

NAMES = list(S.CONFIGS)
MIRROR_NAMES = [n for n in NAMES if S.CONFIGS[n]["mirror"]]
PREDS = (None, "A", "B")


@pytest.mark.parametrize("name", NAMES)
def test_every_step_has_teeth(name):
    """In the float64 model the top 10 (ids and the rows behind them) of at least one checked query, unfiltered or under a checked
    predicate, differs before and after every step."""
    seq = S.sequence(name)
    assert 38 <= len(seq.steps) <= 45

    def tops(snap):
        return [tuple(map(tuple, seq.top(snap, qi, pred))) for qi in range(S.N_QUERIES) for pred in PREDS]

    before = tops(seq.steps[0].after)
    for si, st in enumerate(seq.steps[1:], 1):
        after = tops(st.after)
        assert after != before, f"{name} step {si} ({st.name}) changes no checked answer"
        before = after


@pytest.mark.parametrize("name", NAMES)
def test_every_coverage_class_is_entered(name):
    seq = S.sequence(name)
    tags = seq.tags()
    wanted = S.MIRROR_CLASSES if seq.mirror else S.L2_CLASSES
    assert not [c for c in wanted if c not in tags], tags
    # every operation with staged single adds pending in front of it
    staged = {t.split(":", 1)[1] for t in tags if t.startswith("staged_pending:")}
    assert staged >= set(S.OP_KINDS), staged
    # every kind of store mutation and an attribute change lie between two steps, and every step runs tickets of predicate A
    kinds = {op[0] for st in seq.steps[1:] for op in st.ops}
    assert kinds >= set(S.OP_KINDS), kinds
    # the step that holds exactly 4 096 listed upserts converts those rows only; one more starts the mirror over
    if seq.mirror:
        by = {t: st for st in seq.steps for t in st.tags}
        held, over = by["upserts_4096_listed"], by["upserts_4097_stale"]
        assert held is not over and "upserts_4097_stale" not in held.tags
        distinct = min(S.K_MAX_DIRTY, held.after.count - 5)
        assert held.counters["mirror_rows_converted"] == distinct
        assert over.counters["mirror_rows_converted"] == over.after.count


@pytest.mark.parametrize("name", NAMES)
def test_counter_predictions_restate_the_scripted_rules(name):
    """test_mirror_follows_upserts_removals_growth_and_deserialize, test_id_table_takes_appends_without_a_rebuild and the
    stale_then_rebuilt scripts, on the sequence's own steps."""
    seq = S.sequence(name)
    prev = None
    for si, st in enumerate(seq.steps):
        c, n = st.counters, st.after.count
        kinds = [op[0] for op in S.store_ops(st)]                                     # (the column ops move none of these structures)
        assert 0 <= c["mirror_rows_converted"] <= n and 0 <= c["idhash_rows_inserted"] <= n
        if not seq.mirror:
            assert c["mirror_rows_converted"] == 0 and c["mirror8_conversions"] == 0 and c["mirror8_rows_converted"] == 0
        if si == 0 or "roundtrip" in kinds or "deserialize_blob" in kinds:        # everything is new
            assert c["idhash_rows_inserted"] == n
            if seq.mirror:
                assert c["mirror_rows_converted"] == n and (c["mirror8_conversions"], c["mirror8_rows_converted"]) == (1, n)
        elif set(kinds) <= {"setAttributes"}:                                       # no structure but the attribute columns moves
            assert set(c.values()) == {0}
        elif set(kinds) <= {"remove", "removeBatch"} and n < prev:                  # the tail moved: nothing is converted again,
            assert c["mirror_rows_converted"] == 0 and c["idhash_rows_inserted"] == n            # the id table starts over
            if seq.mirror:
                assert (c["mirror8_conversions"], c["mirror8_rows_converted"]) == (1, n)
        prev = n


@pytest.mark.parametrize("name", MIRROR_NAMES)
def test_nine_in_ten_mirror_answers_certify(name):
    """Per (step, query, k) and mirror, unfiltered and under the predicates the mirror readers use: margin >= MARGIN_FLOOR."""
    seq, mg = S.sequence(name), S.margins(name)
    total, inside, smallest = 0, 0, {8: np.inf, 16: np.inf}
    for si in range(len(seq.steps)):
        for qi in range(S.N_QUERIES):
            for k in S.KS:
                for pred in (None, "A"):
                    m8, m16 = mg.margin8(si, qi, k, pred), mg.margin16(si, qi, k, pred)
                    for bits, m in ((8, m8), (16, m16)):
                        total += 1
                        inside += m >= PM.MARGIN_FLOOR
                        if m >= PM.MARGIN_FLOOR:
                            smallest[bits] = min(smallest[bits], m)
    print(f"\n[{name}] certifying class: {inside} of {total} checked mirror answers; smallest margins inside it: "
          f"8-bit {smallest[8]:.4f}, bf16 {smallest[16]:.4f}")
    assert inside * 10 >= total * 9, (inside, total)


@pytest.mark.parametrize("name", MIRROR_NAMES)
def test_margins_are_the_reference_modules(name):
    """At the first step (where the running maxima are the store's own) the per-row form equals mirror8_planes_ref.margin over
    mirror8_ref.Coded and predicate_mirror_ref.Model.margin."""
    seq, mg = S.sequence(name), S.margins(name)
    snap = seq.steps[0].after
    rows = seq.matrix(snap)
    coded = R8.Coded(rows, seq.metric)
    model = PM.Model(seq.metric, rows, seq.queries)
    everything = np.ones(snap.count, dtype=bool)
    for qi in range(S.N_QUERIES):
        for k in S.KS:
            assert mg.margin8(0, qi, k) == pytest.approx(P8.margin(coded, seq.queries[qi], k), abs=1e-12)
            assert mg.margin16(0, qi, k) == pytest.approx(model.margin(everything, qi, k), abs=1e-12)


@pytest.mark.parametrize("name", NAMES)
def test_two_rows_one_id_resolve_to_the_lower_row(name):
    """The foreign segment parses (the oracle's MV2V reader), the model and helpers.OracleEngine agree on what a call by the shared
    id means: remove takes the lower row and leaves the upper one, which the next upsert overwrites."""
    seq, shared = S.sequence(name), S.shared_id(name)
    si = next(i for i, st in enumerate(seq.steps) if "dup_blob" in st.tags)
    op = S.store_ops(seq.steps[si])[-1]
    blob = S.blob_of(seq, op[1], op[2])
    ref = OracleEngine(seq.metric, seq.dims)
    ref.deserialize(blob)
    snap = seq.steps[si].after
    assert ref.ids == [int(i) for i in snap.ids] and np.array_equal(ref.matrix(), seq.matrix(snap))
    where = np.flatnonzero(snap.ids == np.uint64(shared))
    assert len(where) == 2 and snap.repeated
    lower_row, upper_row = snap.rows[where]
    for st in seq.steps[si + 1: si + 3]:
        for op in st.ops:
            if op[0] == "add":
                ref.add(op[1], seq.pool.rows[op[2]])
            elif op[0] == "removeBatch":
                for fid in op[1]:
                    ref.remove(fid)
        assert ref.ids == [int(i) for i in st.after.ids] and np.array_equal(ref.matrix(), seq.matrix(st.after)), st.name
    after_remove, after_upsert = seq.steps[si + 1].after, seq.steps[si + 2].after
    at = np.flatnonzero(after_remove.ids == np.uint64(shared))
    assert len(at) == 1 and after_remove.rows[at[0]] == upper_row and lower_row not in after_remove.rows
    at2 = np.flatnonzero(after_upsert.ids == np.uint64(shared))
    assert list(at2) == list(at) and after_upsert.rows[at2[0]] != upper_row and after_upsert.count == after_remove.count


@pytest.mark.parametrize("name", NAMES)
def test_model_equals_the_oracle_engine_on_the_whole_sequence(name):
    """The model's store semantics are helpers.OracleEngine's (the reference's), op by op; serialize included."""
    seq = S.sequence(name)
    ref = OracleEngine(seq.metric, seq.dims)
    for st in seq.steps:
        for op in st.ops:
            if op[0] == "addBatch":
                ref.addBatch(op[1], seq.pool.rows[np.asarray(op[2], dtype=np.int64)])
            elif op[0] == "add":
                ref.add(op[1], seq.pool.rows[op[2]])
            elif op[0] == "remove":
                ref.remove(op[1])
            elif op[0] == "removeBatch":
                for fid in op[1]:
                    ref.remove(fid)
            elif op[0] == "roundtrip":
                ref.deserialize(ref.serialize())
            elif op[0] == "deserialize_blob":
                ref.deserialize(S.blob_of(seq, op[1], op[2]))
        assert ref.ids == [int(i) for i in st.after.ids], st.name
        assert np.array_equal(ref.matrix(), seq.matrix(st.after)), st.name


# ---- the per-row columns: timestamps and flags, parents, term sets ------------------------------------------------------------

LANES = ("attrs", "parents", "terms")
TAIL = ["append past every device column", "removal of every row under the columns", "columns again"]
# Steps that move or mark a lane's host column and cannot change one of its checked answers. Step 13 creates both columns with nothing
# in them (every set empty, every parent NO_PARENT): it answers as the step before it, which had no columns. Step 31 of the cosine
# store removes a frame that fails predicate A and is not among the 4096 newest: no checked timeline list holds it.
EMPTY_COLUMNS_STEP = 13
TOOTHLESS_STEPS = {"attrs": {"cos384": (31,)}, "parents": dict.fromkeys(S.CONFIGS, (EMPTY_COLUMNS_STEP,)), "terms": dict.fromkeys(S.CONFIGS, (EMPTY_COLUMNS_STEP,))}


def replay(seq):
    """(step index, op, the model) behind every op, on a fresh Model."""
    m = S.Model()
    for si, st in enumerate(seq.steps):
        for op in st.ops:
            yield si, op, m, False
            S.model_apply(m, op)
            yield si, op, m, True


@pytest.mark.parametrize("name", NAMES)
def test_the_sequences_from_before_the_columns_have_not_moved(name):
    """Store ops, step names and predicted counters of the first BASE_STEPS steps, with what the overlay inserted filtered out, digest to
    what they did before the columns joined; the tail follows them."""
    seq = S.sequence(name)
    assert S.digest(seq.steps[:S.BASE_STEPS]) == S.BASE_DIGESTS[name]
    assert [st.name for st in seq.steps[S.BASE_STEPS:]] == TAIL
    for st in seq.steps:
        assert set(st.counters) == {"mirror_rows_converted", "idhash_rows_inserted", "mirror8_conversions", "mirror8_rows_converted"}
        assert set(st.column_counters) == set(S.COLUMN_COUNTERS)


@pytest.mark.parametrize("name", NAMES)
def test_every_column_class_is_entered(name):
    seq = S.sequence(name)
    tags = seq.tags()
    wanted = S.COLUMN_CLASSES if seq.mirror else S.L2_COLUMN_CLASSES
    assert not [c for c in wanted if c not in tags], sorted(tags)
    assert set(S.INSERT_POSITIONS) <= tags
    staged = {t.split(":", 1)[1] for t in tags if t.startswith("staged_pending:")}
    assert staged >= set(S.COLUMN_OPS)
    by = {t: i for i, st in enumerate(seq.steps) for t in st.tags}
    # the shared id carries all three columns into the removeBatch of the loop path, one step on
    si = by["columns_on_shared_id"]
    snap, shared = seq.steps[si].after, S.shared_id(name)
    lower, upper = np.flatnonzero(snap.ids == np.uint64(shared))
    assert snap.ts[lower] == 3000 and snap.parent[lower] == S.FOREIGN_ROOT0 + 3 and S.SESSIONS[0] in snap.terms[lower]
    assert snap.ts[upper] == 0 and snap.parent[upper] == S.NO_PARENT and snap.terms[upper] == ()
    assert "remove_batch_loop_path" in seq.steps[si + 1].tags and "dup_blob" in seq.steps[si].tags
    # the tail's removal empties all three host columns at once
    gone = seq.steps[by["terms_emptied"]]
    assert by["terms_emptied"] == by["parents_emptied"] and not gone.after.has_terms() and not gone.after.has_parents()
    assert not gone.after.ts.any() and gone.after.count > S.KP


@pytest.mark.parametrize("name", MIRROR_NAMES)
def test_both_required_sets_pass_more_rows_than_the_mirror_rescores(name):
    """R1 and R2 pass more than KP rows (the masked mirror pass then runs) at every step whose store holds a term at all; the steps
    without one — behind a deserialize, behind the removal of every row under the column, and the column of empty sets — are four."""
    seq = S.sequence(name)
    bare = [i for i, st in enumerate(seq.steps) if not st.after.has_terms()]
    assert len(bare) == 3 and all("terms_dropped_by_deserialize" in seq.steps[i].tags or "terms_all_sets_empty" in seq.steps[i].tags
                                  or "terms_emptied" in seq.steps[i].tags for i in bare), bare
    for i, st in enumerate(seq.steps):
        if i not in bare:
            for req in (S.R1, S.R2):
                for pred in (None, "A"):
                    assert int(st.after.mask(pred, req).sum()) > S.KP, (i, st.name, req, pred)
            held = np.array([len(t) > 0 for t in st.after.terms])             # about half the rows that hold terms pass R1, one in eight R2
            assert 0.35 < st.after.term_mask(S.R1)[held].mean() < 0.65 and 0.06 < st.after.term_mask(S.R2)[held].mean() < 0.2


@pytest.mark.parametrize("name", NAMES)
def test_every_column_op_has_teeth(name):
    """Every setTerms moves a current top-10 row of a checked query across R1 or R2; every setParents changes the (10, 3) grouped answer
    of a checked query — but for the two ops of the step that creates the columns with nothing in them."""
    seq = S.sequence(name)
    before, n_ops = None, 0
    for si, op, m, done in replay(seq):
        if op[0] not in S.COLUMN_OPS:
            continue
        if not done:
            before = S.Snapshot(m)
            continue
        after = S.Snapshot(m)
        n_ops += 1
        if si == EMPTY_COLUMNS_STEP:
            assert "terms_all_sets_empty" in seq.steps[si].tags and "parents_all_no_parent" in seq.steps[si].tags
            continue
        if op[0] == "setTerms":
            moved = False
            for qi in range(S.N_QUERIES):
                rows = np.lexsort((np.arange(before.count), seq.pool.exact[before.rows, qi]))[:10]
                moved |= any((before.term_mask(req)[rows] != after.term_mask(req)[rows]).any() for req in (S.R1, S.R2))
            assert moved, (si, seq.steps[si].name, op[1][:4])
        else:
            assert any(seq.grouped(before, qi, None) != seq.grouped(after, qi, None) for qi in range(S.N_QUERIES)), (si, seq.steps[si].name, op[1][:4])
    assert n_ops >= 2 * (S.BASE_STEPS - 8)


@pytest.mark.parametrize("name", NAMES)
def test_every_step_that_moves_a_column_changes_an_answer_of_its_lane(name):
    """A removal below the column's end, a set op, a re-attribution, a deserialize: one of the lane's checked answers on the model (the
    long timeline lists and the (1024, 8) grouped answer included) differs before and after the step. The steps that cannot change one
    are named in TOOTHLESS_STEPS: at most one step in ten per lane."""
    seq = S.sequence(name)
    exempt = {lane: 0 for lane in LANES}
    moved_steps = {lane: 0 for lane in LANES}
    answers = {lane: seq.lane_answers(seq.steps[0].after, lane) for lane in LANES}
    for si, st in enumerate(seq.steps[1:], 1):
        for lane in LANES:
            now = seq.lane_answers(st.after, lane)
            if lane in st.moved:
                moved_steps[lane] += 1
                if si in TOOTHLESS_STEPS[lane].get(name, ()):
                    exempt[lane] += 1
                else:
                    assert now != answers[lane], f"{name} step {si} ({st.name}) moves the {lane} column and changes none of its checked answers"
            answers[lane] = now
    assert all(10 * exempt[lane] <= len(seq.steps) for lane in LANES), exempt
    assert all(moved_steps[lane] >= 20 for lane in LANES), moved_steps


@pytest.mark.parametrize("name", MIRROR_NAMES)
def test_nine_in_ten_term_masked_mirror_answers_certify(name):
    """The bf16 margin of the term-masked answers the GPU test reads on the mirror route: R1 and R2, alone and with predicate A."""
    seq, mg = S.sequence(name), S.margins(name)
    total = inside = 0
    for si, st in enumerate(seq.steps):
        if not st.after.has_terms():
            continue
        for req in (S.R1, S.R2):
            for pred in (None, "A"):
                for qi in range(S.N_QUERIES):
                    for k in S.KS:
                        total += 1
                        inside += mg.margin16(si, qi, k, pred, req) >= PM.MARGIN_FLOOR
    print(f"\n[{name}] certifying class of the term-masked bf16 answers: {inside} of {total}")
    assert inside * 10 >= total * 9, (inside, total)


class ParentModel:
    """The Model of tests/test_grouped_gpu.py restated (a test module is not imported from another): rows in order, each (frame id, parent)."""

    def __init__(self):
        self.ids, self.parents = [], []

    def add(self, ids):
        for i in ids:
            if i not in self.ids:                                # an upsert keeps its row and its parent
                self.ids.append(i); self.parents.append(S.NO_PARENT)   # an appended row is its own root

    def set_parents(self, ids, parents):
        for i, p in zip(ids, parents):
            if i in self.ids:
                self.parents[self.ids.index(i)] = int(p)

    def remove(self, ids):
        for i in ids:
            if i in self.ids:
                at = self.ids.index(i)
                del self.ids[at], self.parents[at]

    def replace(self, ids):
        self.ids, self.parents = list(ids), [S.NO_PARENT] * len(ids)


@pytest.mark.parametrize("name", NAMES)
def test_column_semantics_equal_the_lane_models(name):
    """terms_ref.StoreModel and the grouped lane's Model, op by op: an appended row takes the defaults, an upsert keeps its entries, a
    removal takes them, deserialize drops them, a set skips ids not held, its last entry of a repeated id wins, a shared id names the
    lower row."""
    import terms_ref
    seq, shared = S.sequence(name), S.shared_id(name)
    tm, pm = terms_ref.StoreModel(1), ParentModel()
    shared_sets = 0
    for st in seq.steps:
        for op in st.ops:
            kind = op[0]
            ids = [int(i) for i in op[1]] if kind in ("addBatch", "removeBatch", "setParents", "setTerms") else None
            if kind in ("addBatch", "add"):
                ids = ids if kind == "addBatch" else [int(op[1])]
                tm.add_batch(ids, np.zeros((len(ids), 1), dtype=np.float32))
                pm.add(ids)
            elif kind == "remove":
                tm.remove(op[1]); pm.remove([int(op[1])])
            elif kind == "removeBatch":
                if len(set(tm.ids)) != len(tm.ids):              # the per-id loop, in call order
                    for f in ids:
                        tm.remove(f)
                else:
                    tm.remove_batch(ids)
                pm.remove(ids)
            elif kind in ("roundtrip", "deserialize_blob"):
                new = list(tm.ids) if kind == "roundtrip" else [int(i) for i in op[1]]
                tm.ids, tm.rows = list(new), [np.zeros(1, dtype=np.float32)] * len(new)
                tm.drop_terms()
                pm.replace(new)
            elif kind == "setTerms":
                tm.set_terms(ids, op[2])
                shared_sets += shared in ids and tm.ids.count(shared) == 2
            elif kind == "setParents":
                pm.set_parents(ids, op[2])
                shared_sets += shared in ids and pm.ids.count(shared) == 2
        snap = st.after
        assert tm.ids == pm.ids == [int(i) for i in snap.ids], st.name
        assert [tuple(s) for s in tm.sets] == snap.terms, st.name
        assert pm.parents == [int(p) for p in snap.parent], st.name
    assert shared_sets == 2                                      # both lanes named the shared id while two rows held it
    # ids not held and repeated ids occur among the column ops
    ops = [(si, op) for si, st in enumerate(seq.steps) for op in st.ops if op[0] in S.COLUMN_OPS]
    assert any(len(set(op[1])) != len(op[1]) for _, op in ops)


@pytest.mark.parametrize("name", NAMES)
def test_column_counter_predictions_restate_the_scripted_rules(name):
    """What test_lifecycle_follows_a_rebuilt_store and test_lifecycle_follows_the_other_columns script, on the sequence's own steps: an
    unchanged step uploads nothing, the first setParents and the first term read upload `count` rows, a change uploads the rows from the
    lowest changed (or first appended) row on, after deserialize nothing is uploaded and the term searches are decided on the host."""
    seq = S.sequence(name)
    first = seq.steps[0]
    n0 = first.after.count
    assert first.column_counters["parent_rows_uploaded"] == n0 and first.column_counters["term_rows_uploaded"] == n0
    assert first.column_counters["term_values_uploaded"] == sum(len(s) for s in first.after.terms)
    # the lowest row each lane's ops marked, per step, from a replay of the model alone
    lowest = [{"parents": None, "terms": None} for _ in seq.steps]
    for si, op, m, done in replay(seq):
        if done:
            continue
        rows = []
        if op[0] == "remove":
            rows = [m.find(int(op[1]))]
        elif op[0] == "removeBatch":
            rows = [m.find(int(f)) for f in op[1]] if not m.has_repeated_ids() else [m.find(int(op[1][0]))]
        elif op[0] in S.COLUMN_OPS:
            rows, lane = [m.find(int(f)) for f in op[1]], "parents" if op[0] == "setParents" else "terms"
            rows = [r for r in rows if r >= 0]
            if rows:
                lowest[si][lane] = min(rows + ([lowest[si][lane]] if lowest[si][lane] is not None else []))
            continue
        for lane in ("parents", "terms"):
            rows = [r for r in rows if r >= 0]
            if rows:
                lowest[si][lane] = min(rows + ([lowest[si][lane]] if lowest[si][lane] is not None else []))
    prev = None
    for si, st in enumerate(seq.steps):
        c, n, kinds = st.column_counters, st.after.count, {op[0] for op in st.ops}
        assert 0 <= c["parent_rows_uploaded"] <= n and 0 <= c["term_rows_uploaded"] <= n
        assert c["term_values_uploaded"] <= sum(len(s) for s in st.after.terms)
        # the slot count: at least the distinct roots present, at most what starts the numbering over
        roots = len(set(S.GR.roots_of(st.after.parent, st.after.ids).tolist()))
        assert roots <= c["group_slots"] <= 2 * n + 16, (si, st.name)
        if not st.after.has_parents() and "parents_all_no_parent" not in st.tags:
            assert c["group_slots"] == n and c["parent_rows_uploaded"] == 0
        if kinds <= {"setAttributes"}:                           # an unchanged step uploads nothing
            assert (c["parent_rows_uploaded"], c["term_rows_uploaded"], c["term_values_uploaded"]) == (0, 0, 0), (si, st.name)
        if kinds & {"roundtrip", "deserialize_blob"} and not kinds & set(S.COLUMN_OPS):
            assert (c["parent_rows_uploaded"], c["term_rows_uploaded"], c["term_values_uploaded"]) == (0, 0, 0) and not st.after.has_terms()
        special = st.tags & {"parents_first_set", "parents_growth_whole_column", "parents_renumber_from_scratch", "parents_dropped_by_deserialize", "parents_emptied"}
        if prev is not None and prev.after.has_parents() and not special and si != 0:
            low = min(prev.after.count, n if lowest[si]["parents"] is None else lowest[si]["parents"])
            assert c["parent_rows_uploaded"] == n - min(low, n), (si, st.name, low)
        special = st.tags & {"terms_first_upload", "terms_value_growth_keeps_prefix", "terms_offset_growth_keeps_prefix", "terms_dropped_by_deserialize", "terms_emptied"}
        if prev is not None and prev.after.has_terms() and not special:
            low = min(prev.after.count, n if lowest[si]["terms"] is None else lowest[si]["terms"])
            assert c["term_rows_uploaded"] == n - min(low, n), (si, st.name, low)
        prev = st
    by = {t: st for st in seq.steps for t in st.tags}
    grown = by["parents_growth_whole_column"]
    assert grown.column_counters["parent_rows_uploaded"] == grown.after.count           # the slot column is sent again whole
    kept = by["terms_offset_growth_keeps_prefix"]
    assert 0 < kept.column_counters["term_rows_uploaded"] < kept.after.count            # the term arrays keep what was current
    kept = by["terms_value_growth_keeps_prefix"]
    assert 0 < kept.column_counters["term_rows_uploaded"] < kept.after.count


@pytest.mark.parametrize("name", NAMES)
def test_the_vectorised_lane_models_are_the_lane_models(name):
    """The GPU test takes its expected timeline from Sequence.timeline, its expected grouped answer from grouped_answer and its term
    masks from terms_ref.pass_csr (the lane models loop over the rows in Python: thirteen readers per step cannot afford them). Here they
    equal timeline_ref.timeline_model, grouped_ref.grouped_model and terms_ref.pass_set on the sequence's own stores, under every
    predicate and limit the GPU test asks, on keys with ties."""
    import grouped_ref as GR
    import timeline_ref as TL
    from terms_ref import pass_set as TL_pass_set
    seq = S.sequence(name)
    rng = np.random.default_rng(7)
    for si in range(0, len(seq.steps), 6):
        snap = seq.steps[si].after
        for req in (S.R1, S.R2, (S.EVERYBODY,), (5,)):
            assert np.array_equal(snap.term_mask(req), TL_pass_set(snap.terms, req)), (si, req)
        if snap.repeated:
            continue                                             # (timeline_model asks for unique ids)
        for newest in (True, False):
            for pred in (None, "A", "B"):
                kw = S.PREDICATES[pred] if pred else {}
                after, before = kw.get("timeRange", (None, None))
                for limit in (1, 300, 4096):
                    exp = TL.timeline_model(snap.ts, snap.fl, snap.ids, limit, newest, after, before, kw.get("denyFlags", 0))
                    got = seq.timeline(snap, limit, newest, pred)
                    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]), (si, newest, pred, limit)
        dist = seq.pool.exact[snap.rows, 0].astype(np.float32)
        dist[rng.integers(0, snap.count, 200)] = dist[rng.integers(0, snap.count, 200)]      # equal bits across and inside groups
        dist[rng.integers(0, snap.count, 3)] = np.inf
        keys = GR.make_keys(dist)
        for pred in (None, "A", "B"):
            passing = None if pred is None else snap.mask(pred)
            for limit, per_group in ((10, 3), (1024, 8), (1, 1)):
                exp = GR.grouped_model(keys, snap.parent, snap.ids, passing, limit, per_group)
                got = S.grouped_answer(keys, snap.parent, snap.ids, passing, limit, per_group)
                for a, b in zip(got, exp):
                    assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (si, pred, limit, per_group)
