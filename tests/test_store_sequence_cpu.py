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
        kinds = [op[0] for op in st.ops]
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
    op = seq.steps[si].ops[-1]
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
