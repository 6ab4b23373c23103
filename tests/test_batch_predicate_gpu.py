"""Batched predicate search (wax_hip_search_batch_predicate / searchBatchFiltered with timeRange and denyFlags): every row must equal
what searchFiltered returns for that query, its allow-list, its predicate and its cut — ids, scores and counts bit for bit — and the
counters must show that the batched gather pass answered it, so that a fallback cannot hide a wrong pass.

The reference of every equality test is the single-query path, looped. Stores are the smallest at which the kernels can go wrong:
one row, the wave (64), the tile (256), the 4 096-row work item and their neighbours, several work items, several query groups."""
import ctypes
import threading

import numpy as np
import pytest

import oracle
from helpers import assert_parity

pytestmark = pytest.mark.gpu

COUNTERS = ("filter_batch_fallbacks", "filter_batch_queries", "predicate_batch_queries", "predicate_batch_classes", "predicate_searches",
            "filter_device_searches")
TS0 = 1000   # timestamp of row 0; timestamps ascend with the row


@pytest.fixture(scope="module")
def wax(hip_lib):
    import wax_amd
    if hip_lib.wax_hip_device_count() == 0:
        pytest.skip("no HIP device on this host: the gpu-marked tests run on the MI355X box (pytest -m gpu)")
    assert hip_lib.wax_hip_available() == 1, "a HIP device is visible but it is not gfx950: the HIP path needs an MI355X"
    return wax_amd


def corpus_for(metric, n, dims, seed=0):
    x = oracle.gaussian_unit_rows(seed, n, dims)
    if metric == 1:   # dot: rows of different norms
        x = x * np.random.default_rng(seed + 7).uniform(0.5, 2.0, size=(n, 1)).astype(np.float32)
    return np.ascontiguousarray(x, dtype=np.float32)


def make_engine(wax, metric, dims, corpus=None, attrs=True, seed=1, **kw):
    """Rows 0 .. n-1 with frame id = row, timestamp TS0 + row, and one of the three status bits on a random 1/16 of the rows."""
    eng = wax.HIPVectorEngine(metric=wax.VectorMetric(metric), dimensions=dims, **kw)
    n = 0 if corpus is None else len(corpus)
    ts = TS0 + np.arange(n, dtype=np.int64)
    flags = np.zeros(n, dtype=np.uint32)
    if n:
        eng.addBatch(np.arange(n, dtype=np.uint64), corpus)
        rng = np.random.default_rng(seed)
        hit = rng.choice(n, size=n // 16, replace=False)
        flags[hit] = rng.choice(np.array([1, 2, 4], dtype=np.uint32), size=hit.size)
        if attrs:
            assert eng.setAttributes(np.arange(n, dtype=np.uint64), ts, flags) == n
    return eng, ts, flags


def random_list(rng, n_rows, length):
    """`length` ids of which ~5 % are not in the engine (ids >= n_rows) and a few repeat."""
    if length == 0:
        return np.zeros(0, dtype=np.uint64)
    if length >= n_rows:
        ids = rng.permutation(n_rows).astype(np.uint64)
    else:
        ids = rng.choice(n_rows, size=length, replace=False).astype(np.uint64)
    m = max(1, length // 20) if length > 1 else 0
    if m:
        ids[:m] = rng.integers(n_rows, 2 * n_rows + 10 ** 6, size=m, dtype=np.uint64)       # absent ids
        ids[m:2 * m] = ids[len(ids) - m:] if len(ids) >= 3 * m else ids[m:2 * m]             # duplicates
    return rng.permutation(ids)


def six_predicates(n):
    """(timeRange, denyFlags) x 6 for a store of n rows made by make_engine: the middle third, the status bits, both, nothing,
    everything through a bound that is set, the last row alone."""
    mid = (TS0 + n // 3, TS0 + (2 * n) // 3)
    return [(mid, 0), (None, 0b111), (mid, 0b111), ((None, TS0 - 1), 0), ((TS0, None), 0), ((TS0 + n - 1, None), 0)]


def is_effective(pred):
    rng, deny = pred
    return bool(deny) or (rng is not None and (rng[0] is not None or rng[1] is not None))


def passes(pred, ts, flags):
    rng, deny = pred
    m = (flags & np.uint32(deny)) == 0
    if rng is not None and rng[0] is not None:
        m &= ts >= rng[0]
    if rng is not None and rng[1] is not None:
        m &= ts < rng[1]
    return m


def loop(eng, queries, k, preds, lists=None, cuts=None):
    out = []
    for q in range(len(queries)):
        out.append(eng.searchFiltered(queries[q], k, frameIds=None if lists is None else lists[q], minScore=None if cuts is None else cuts[q],
                                      timeRange=preds[q][0], denyFlags=preds[q][1]))
    return out


def batch(eng, queries, k, preds, lists=None, cuts=None):
    return eng.searchBatchFiltered(queries, k, frameIds=lists, minScore=cuts, timeRange=[p[0] for p in preds], denyFlags=[p[1] for p in preds])


def assert_rows_equal(got, ref, ctx):
    ids, scores, counts = got
    for q, (ri, rs) in enumerate(ref):
        n = int(counts[q])
        assert n == len(ri), f"{ctx}: query {q} count {n} != {len(ri)}"
        assert np.array_equal(ids[q, :n], ri), f"{ctx}: query {q} ids"
        assert np.array_equal(scores[q, :n], rs), f"{ctx}: query {q} scores"


def snap(eng):
    return {key: eng.getTuning(key) for key in COUNTERS}


def assert_pass(eng, before, taken, with_pred, ctx, classes=None, fallbacks=0):
    """The batched pass took `taken` queries, `with_pred` of them with an effective predicate; `fallbacks` took the single-query body."""
    d = {key: eng.getTuning(key) - before[key] for key in COUNTERS}
    assert d["filter_batch_fallbacks"] == fallbacks, f"{ctx}: {d}"
    assert d["predicate_batch_queries"] == with_pred, f"{ctx}: {d}"
    assert d["filter_batch_queries"] == taken, f"{ctx}: {d}"
    if classes is not None:
        assert d["predicate_batch_classes"] == classes, f"{ctx}: {d}"
    return d


def checked_batch(eng, queries, k, preds, ctx, lists=None, cuts=None, classes=None):
    """One batched call whose every query the pass must take, compared with the loop."""
    before = snap(eng)
    got = batch(eng, queries, k, preds, lists, cuts)
    taken = sum(1 for q in range(len(queries)) if is_effective(preds[q]) or (lists is not None and lists[q] is not None))
    assert_pass(eng, before, taken, sum(1 for p in preds if is_effective(p)), ctx, classes)
    assert_rows_equal(got, loop(eng, queries, k, preds, lists, cuts), ctx)
    return got


def raw_call(eng, queries, k, preds=None, lists=None, stride=None, filtered_entry=False):
    """The C entry itself: `preds` is None or a list of (has_after, after, has_before, before, deny_flags) as they go into the struct."""
    from wax_amd import _abi
    from wax_amd.engine import pack_allow_lists
    lib = _abi.lib()
    u64, f32, u32 = (ctypes.POINTER(t) for t in (ctypes.c_uint64, ctypes.c_float, ctypes.c_uint32))
    qs = np.ascontiguousarray(queries, np.float32)
    nq, dims = qs.shape
    stride = stride or max(1, min(k, eng.count))
    flat, begin, length = pack_allow_lists(lists, nq)
    ids, scores, counts = np.zeros((nq, stride), np.uint64), np.zeros((nq, stride), np.float32), np.zeros(nq, np.uint32)
    arr = None
    if preds is not None:
        arr = (_abi.RowPredicate * nq)(*[_abi.RowPredicate(*p) for p in preds])
    head = (eng._h, qs.ctypes.data_as(f32), nq, dims, k, None if flat.size == 0 else flat.ctypes.data_as(u64), int(flat.size),
            None if begin is None else begin.ctypes.data_as(u64), None if length is None else length.ctypes.data_as(u64), None)
    tail = (ids.ctypes.data_as(u64), scores.ctypes.data_as(f32), stride, counts.ctypes.data_as(u32))
    rc = lib.wax_hip_search_batch_filtered(*head, *tail) if filtered_entry else lib.wax_hip_search_batch_predicate(*head, arr, *tail)
    return rc, ids, scores, counts


# ---- 1. edge sizes of the column -> row-list kernels -------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", [0, 1, 2], ids=["cosine", "dot", "l2"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257, 4095, 4096, 4097, 8193, 40000])
def test_edge_sizes_of_the_row_list_kernels(wax, n, metric):
    """k = 150 is the `k larger than the passing rows`: above every store up to 65 rows, above the last-row and the empty predicate
    everywhere, and still inside the batched pass (top_k <= 192)."""
    dims = 64
    eng, _, _ = make_engine(wax, metric, dims, corpus_for(metric, n, dims, seed=n), seed=n)
    vectors = oracle.gaussian_unit_queries(8, dims)
    preds = [p for p in six_predicates(n) for _ in range(8)]
    queries = np.ascontiguousarray(np.concatenate([vectors] * 6), dtype=np.float32)
    for k in (1, 10, 150):
        got = checked_batch(eng, queries, k, preds, f"n={n} metric={metric} k={k}", classes=len(set(preds)))   # (one row: two of the six coincide)
        assert (got[2][24:32] == 0).all()                       # the predicate that passes nothing
        assert (got[2][40:48] == 1).all() and (got[0][40:48, 0] == n - 1).all()   # ... only the last row
    eng.close()


# ---- 2. dims and multi-item splits ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,dims", [(100_000, 384), (30_000, 768)], ids=["100k_384", "30k_768"])
def test_dims_and_several_work_items(wax, n, dims):
    eng, _, _ = make_engine(wax, 0, dims, corpus_for(0, n, dims, seed=2))
    queries = oracle.gaussian_unit_queries(64, dims)
    four = [six_predicates(n)[i] for i in (0, 1, 2, 4)]
    preds = [four[q % 4] for q in range(64)]
    for k in (10, 100, 192):
        if dims >= 512 and k > 60:
            # the gather kernel keeps 16 lists per wave in LDS and serves k <= 60 from 512-d up (scan_multi_group): the call falls
            # back as wax_hip_search_batch_filtered does there, and says so
            assert eng.getTuning("batch_multi_group_big") == 0
            before = snap(eng)
            got = batch(eng, queries, k, preds)
            assert_pass(eng, before, 0, 0, f"{n}x{dims} k={k}", classes=0, fallbacks=64)
            assert_rows_equal(got, loop(eng, queries, k, preds), f"{n}x{dims} k={k}")
        else:
            checked_batch(eng, queries, k, preds, f"{n}x{dims} k={k}", classes=4)
    eng.close()


# ---- the 40 000 x 64 store most of the remaining tests share ----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def store(wax):
    n, dims = 40_000, 64
    corpus = corpus_for(0, n, dims, seed=5)
    eng, ts, flags = make_engine(wax, 0, dims, corpus, seed=5)
    yield eng, corpus, ts, flags
    eng.close()


# ---- 3. lists AND predicates ------------------------------------------------------------------------------------------------------

def test_lists_and_predicates(wax, store):
    eng, corpus, _, _ = store
    n = len(corpus)
    rng = np.random.default_rng(3)
    lengths = [0, 1, 64, 65, 4095, 4096, 16384, 16385]           # the last one is too long for the LDS sort: the bitmap route
    made = [random_list(rng, n, length) for length in lengths]
    three = [six_predicates(n)[i] for i in (0, 1, 2)]
    lists = [lst for lst in made for _ in three]
    preds = [p for _ in made for p in three]
    queries = oracle.gaussian_unit_queries(len(lists), 64)
    before = snap(eng)
    # the same list object under three predicates is ONE (begin, len) and three entries: 7 lists that allow something x 3
    checked_batch(eng, queries, 10, preds, "lists and predicates", lists=lists, classes=21)
    assert eng.getTuning("filter_device_searches") - before["filter_device_searches"] >= 3   # the long list, once per predicate
    checked_batch(eng, queries, 150, preds, "lists and predicates k=150", lists=lists, classes=21)
    # a list without a predicate beside the same list with one, and a predicate without a list
    mixed_preds = [three[0], (None, 0), three[1], (None, 0), three[2], (None, 0)]
    mixed_lists = [made[4], made[4], made[7], made[7], None, made[2]]
    checked_batch(eng, queries[:6], 10, mixed_preds, "mixed", lists=mixed_lists, classes=3)


# ---- 4. sharing -------------------------------------------------------------------------------------------------------------------

def test_queries_share_entries_by_normalised_predicate(wax, store):
    eng, corpus, _, _ = store
    n = len(corpus)
    a, b = TS0 + n // 4, TS0 + n // 2
    # three predicates, each written with different garbage in the bounds it does not use
    forms = [[(1, a, 0, 111, 0), (1, a, 0, -5, 0), (7, a, 0, 2 ** 40, 0)],
             [(0, 9, 1, b, 0b10), (0, -9, 1, b, 0b10)],
             [(0, 1, 0, 2, 0b101), (0, 3, 0, 4, 0b101), (0, 0, 0, 0, 0b101)]]
    nq = 40
    queries = oracle.gaussian_unit_queries(nq, 64)
    raw = [forms[q % 3][(q // 3) % len(forms[q % 3])] for q in range(nq)]
    clean = [((a, None), 0), ((None, b), 0b10), (None, 0b101)]
    before = snap(eng)
    rc, ids, scores, counts = raw_call(eng, queries, 10, preds=raw)
    assert rc == 0
    assert_pass(eng, before, nq, nq, "sharing", classes=3)
    assert_rows_equal((ids, scores, counts), loop(eng, queries, 10, [clean[q % 3] for q in range(nq)]), "sharing")


# ---- 5. against the oracle, not against the code's other path -----------------------------------------------------------------------

@pytest.mark.parametrize("metric", [0, 1, 2], ids=["cosine", "dot", "l2"])
def test_against_the_oracle(wax, metric):
    n, dims, k = 3000, 384, 10
    corpus = corpus_for(metric, n, dims, seed=9)
    eng, ts, flags = make_engine(wax, metric, dims, corpus, seed=9)
    frame_ids = np.arange(n, dtype=np.uint64)
    queries = oracle.gaussian_unit_queries(18, dims)
    preds = [six_predicates(n)[q % 6] for q in range(18)]
    before = snap(eng)
    ids, scores, counts = batch(eng, queries, k, preds)
    assert_pass(eng, before, 18, 18, f"oracle metric={metric}")
    checked = 0
    for q in range(18):
        mask = passes(preds[q], ts, flags)
        c = int(counts[q])
        assert c == min(k, int(mask.sum())), f"query {q}: {c} results, {int(mask.sum())} rows pass"
        if c == 0:
            continue
        ei, es, _, _ = oracle.search(metric, corpus[mask], frame_ids[mask], queries[q], k)
        _, es_all, _, _ = oracle.search(metric, corpus[mask], frame_ids[mask], queries[q], 2 * k)
        assert_parity(ids[q, :c], scores[q, :c], ei, es, all_exp_scores=es_all, ctx=f"metric {metric} query {q}")
        checked += 1
    assert checked == 15
    eng.close()


# ---- 6. ties ------------------------------------------------------------------------------------------------------------------------

def test_ties_across_a_work_item_boundary_come_in_row_order(wax):
    n, dims = 9000, 64
    corpus = corpus_for(0, n, dims, seed=6)
    twins = list(range(4090, 4102)) + list(range(8188, 8196))    # straddle rows 4096 and 8192
    corpus[twins] = corpus[17]
    eng = wax.HIPVectorEngine(metric=wax.VectorMetric(0), dimensions=dims)
    eng.addBatch(np.arange(n, dtype=np.uint64), corpus)
    flags = np.zeros(n, dtype=np.uint32)
    flags[[17, 4095, 4096, 8191]] = 1
    eng.setAttributes(np.arange(n, dtype=np.uint64), TS0 + np.arange(n, dtype=np.int64), flags)
    queries = np.ascontiguousarray(np.stack([corpus[17]] * 3), dtype=np.float32)
    preds = [(None, 1), ((TS0 + 4093, None), 1), ((TS0 + 4000, TS0 + 8190), 0)]
    got = checked_batch(eng, queries, 16, preds, "ties", classes=3)
    keep = [r for r in twins if r not in (4095, 4096, 8191)]
    assert got[0][0, :16].tolist() == keep[:16]
    late = [r for r in keep if r >= 4093]
    assert len(late) == 14 and got[0][1, :14].tolist() == late
    assert got[0][2, :14].tolist() == [r for r in twins if r < 8190]
    eng.close()


# ---- 7. no attributes set -----------------------------------------------------------------------------------------------------------

def test_a_store_without_attributes_decides_on_the_host(wax):
    n, dims = 5000, 64
    eng, _, _ = make_engine(wax, 0, dims, corpus_for(0, n, dims, seed=7), attrs=False)
    queries = oracle.gaussian_unit_queries(12, dims)
    rng = np.random.default_rng(7)
    lists = [None if q % 2 else random_list(rng, n, 300) for q in range(12)]
    before = snap(eng)
    deny = eng.searchBatchFiltered(queries, 10, frameIds=lists, denyFlags=0b111)        # every row reads (0, 0): passes
    d = assert_pass(eng, before, 6, 0, "deny on a store without attributes", classes=0)  # the six lists; the rest is the plain sub-batch
    assert d["predicate_searches"] == 0
    plain = eng.searchBatchFiltered(queries, 10, frameIds=lists)
    assert all(np.array_equal(x, y) for x, y in zip(deny, plain))
    assert_rows_equal(deny, loop(eng, queries, 10, [(None, 0b111)] * 12, lists), "deny on a store without attributes")
    before = snap(eng)
    _, _, counts = eng.searchBatchFiltered(queries, 10, frameIds=lists, timeRange=(1, None))   # 0 >= 1 fails in every row
    assert (counts == 0).all()
    d = assert_pass(eng, before, 0, 0, "after = 1 on a store without attributes", classes=0)
    assert d["predicate_searches"] == 0
    assert all(len(i) == 0 for i, _ in loop(eng, queries, 10, [((1, None), 0)] * 12, lists))
    eng.close()


# ---- 8. freshness -------------------------------------------------------------------------------------------------------------------

def test_writes_just_before_the_call_are_seen(wax):
    n, dims = 6000, 64
    corpus = corpus_for(0, n + 1, dims, seed=8)
    eng, ts, flags = make_engine(wax, 0, dims, corpus[:n], seed=8)
    queries = np.ascontiguousarray(np.concatenate([oracle.gaussian_unit_queries(5, dims), corpus[[10, 4100, n]]]), dtype=np.float32)
    preds = [((TS0 + 5, None), 0b111)] * 4 + [(None, 0b111)] * 4
    checked_batch(eng, queries, 10, preds, "before the writes")
    # setAttributes: the best rows of queries 5 and 6 are denied (row 10 also leaves the window); row 30 is cleared for the upsert below
    eng.setAttributes(np.array([10, 4100, 30], dtype=np.uint64), np.array([0, TS0 + 4100, TS0 + 30], dtype=np.int64), np.array([4, 1, 0], dtype=np.uint32))
    got = checked_batch(eng, queries, 10, preds, "after setAttributes")
    assert 10 not in got[0][5, :got[2][5]] and 4100 not in got[0][6, :got[2][6]]
    # an upsert keeps the row's attributes and changes its vector
    eng.add(30, corpus[n])
    got = checked_batch(eng, queries, 10, preds, "after an upsert")
    assert got[0][7, 0] == 30
    # an appended row has (0, 0): outside the window of the first four, inside the deny-only predicate of the rest
    eng.add(n, corpus[n])
    got = checked_batch(eng, queries, 10, preds, "after an append")
    assert got[0][7, :2].tolist() == [30, n] and n not in got[0][0, :got[2][0]]
    # removeBatch takes rows and their attributes along
    assert eng.removeBatch(np.array([30, 5, 4097], dtype=np.uint64)) == 3
    got = checked_batch(eng, queries, 10, preds, "after removeBatch")
    assert got[0][7, 0] == n
    eng.close()


# ---- 9. without predicates it is the old call -----------------------------------------------------------------------------------------

def test_without_predicates_it_is_the_old_call(wax):
    n, dims = 20_000, 64
    corpus = corpus_for(0, n, dims, seed=10)
    a, _, _ = make_engine(wax, 0, dims, corpus, seed=10)
    b, _, _ = make_engine(wax, 0, dims, corpus, seed=10)
    rng = np.random.default_rng(10)
    made = [random_list(rng, n, length) for length in (0, 50, 5000, 17000)]
    lists = [None if q % 5 == 4 else made[q % 4] for q in range(30)]
    queries = oracle.gaussian_unit_queries(30, dims)
    for preds in (None, [(0, 5, 0, 6, 0)] * 30):                  # no array at all; an array of predicates that test nothing
        before_a, before_b = snap(a), snap(b)
        stats_a, stats_b = a.stats(), b.stats()
        rc, ids, scores, counts = raw_call(a, queries, 10, preds=preds, lists=lists)
        rc_b, ids_b, scores_b, counts_b = raw_call(b, queries, 10, lists=lists, filtered_entry=True)
        assert rc == 0 and rc_b == 0
        assert np.array_equal(ids, ids_b) and np.array_equal(scores, scores_b) and np.array_equal(counts, counts_b)
        da = {key: a.getTuning(key) - before_a[key] for key in COUNTERS}
        db = {key: b.getTuning(key) - before_b[key] for key in COUNTERS}
        assert da == db, (da, db)
        assert da["filter_batch_queries"] == 24 and da["filter_device_searches"] == 1    # the 17 000-id list: one entry, resolved once
        assert da["predicate_batch_queries"] == 0 and da["predicate_batch_classes"] == 0 and da["predicate_searches"] == 0
        sa, sb = a.stats(), b.stats()
        assert sa.rows_scanned - stats_a.rows_scanned == sb.rows_scanned - stats_b.rows_scanned
        assert sa.bytes_scanned - stats_a.bytes_scanned == sb.bytes_scanned - stats_b.bytes_scanned
        assert sa.searches - stats_a.searches == sb.searches - stats_b.searches
    a.close()
    b.close()


# ---- 10. fallbacks ------------------------------------------------------------------------------------------------------------------

def fallback_case(eng, n, dims, k, ctx, expect_fallbacks=12):
    rng = np.random.default_rng(12)
    queries = oracle.gaussian_unit_queries(12, dims)
    three = [six_predicates(n)[i] for i in (0, 1, 2)]
    preds = [three[q % 3] for q in range(12)]
    lists = [None if q % 2 else random_list(rng, n, 700) for q in range(12)]
    before = snap(eng)
    got = batch(eng, queries, k, preds, lists)
    d = assert_pass(eng, before, 0, 0, ctx, classes=0, fallbacks=expect_fallbacks)
    assert d["predicate_searches"] == 12, d
    assert_rows_equal(got, loop(eng, queries, k, preds, lists), ctx)


def test_unspecialised_dims_fall_back(wax):
    eng, _, _ = make_engine(wax, 0, 100, corpus_for(0, 5000, 100, seed=11))
    fallback_case(eng, 5000, 100, 10, "dims 100")
    eng.close()


def test_large_k_and_switches_fall_back(wax, store):
    eng, corpus, _, _ = store
    fallback_case(eng, len(corpus), 64, 193, "top_k 193")
    for key, value, back in (("filter_batch", 0, 1), ("force_general", 1, 0)):
        eng.setTuning(key, value)
        try:
            fallback_case(eng, len(corpus), 64, 10, key)
        finally:
            eng.setTuning(key, back)


def test_the_row_budget_admits_entries_in_query_order(wax):
    n, dims = 4000, 64
    eng, _, _ = make_engine(wax, 0, dims, corpus_for(0, n, dims, seed=13))
    assert eng.getTuning("predicate_batch_rows") == 2 ** 26
    queries = oracle.gaussian_unit_queries(12, dims)
    three = [six_predicates(n)[i] for i in (0, 1, 2)]
    preds = [three[q % 3] for q in range(12)]
    eng.setTuning("predicate_batch_rows", n + n // 2)            # one entry without a list costs n slots: the first fits, two do not
    before = snap(eng)
    got = batch(eng, queries, 10, preds)
    d = assert_pass(eng, before, 4, 4, "budget", classes=1, fallbacks=8)
    assert d["predicate_searches"] == 12
    assert_rows_equal(got, loop(eng, queries, 10, preds), "budget")
    eng.setTuning("predicate_batch_rows", 2 ** 26)
    checked_batch(eng, queries, 10, preds, "budget restored", classes=3)
    with pytest.raises(Exception):
        eng.setTuning("predicate_batch_rows", -1)
    eng.close()


# ---- 11. cuts -----------------------------------------------------------------------------------------------------------------------

def test_score_cuts_on_top_of_predicates(wax, store):
    eng, corpus, _, _ = store
    n = len(corpus)
    rng = np.random.default_rng(14)
    nq = 30
    queries = np.ascontiguousarray(corpus[rng.choice(n, nq, replace=False)] + 0.3 * oracle.gaussian_unit_queries(nq, 64), dtype=np.float32)
    three = [six_predicates(n)[i] for i in (0, 1, 2)]
    preds = [three[q % 3] for q in range(nq)]
    lists = [None if q % 2 else random_list(rng, n, 3000) for q in range(nq)]
    cuts = [[None, 0.3, float("nan"), float("inf"), -1.0][q % 5] for q in range(nq)]
    got = checked_batch(eng, queries, 10, preds, "cuts", lists=lists, cuts=cuts)
    assert all(got[2][q] == 0 for q in range(nq) if cuts[q] == float("inf"))
    assert any(0 < got[2][q] < 10 for q in range(nq) if cuts[q] == 0.3)      # the cut bites somewhere, and not everywhere


# ---- 12. out_stride < k, and what the call refuses ------------------------------------------------------------------------------------

def test_out_stride_below_k_keeps_the_best(wax, store):
    eng, corpus, _, _ = store
    n = len(corpus)
    queries = oracle.gaussian_unit_queries(9, 64)
    three = [six_predicates(n)[i] for i in (0, 1, 2)]
    preds = [three[q % 3] for q in range(9)]
    lists = [None if q < 6 else np.arange(0, n, 3, dtype=np.uint64) for q in range(9)]
    full = loop(eng, queries, 40, preds, lists)
    raw = [(0 if p[0] is None else 1, 0 if p[0] is None else p[0][0], 0 if p[0] is None else 1, 0 if p[0] is None else p[0][1], p[1]) for p in preds]
    before = snap(eng)
    rc, ids, scores, counts = raw_call(eng, queries, 40, preds=raw, lists=lists, stride=7)
    assert rc == 0
    assert_pass(eng, before, 9, 9, "stride 7")
    for q in range(9):
        assert counts[q] == 7 and np.array_equal(ids[q], full[q][0][:7]) and np.array_equal(scores[q], full[q][1][:7])


def test_refusals(wax, store):
    from wax_amd import _abi
    eng = store[0]
    lib = _abi.lib()
    u64, f32, u32 = (ctypes.POINTER(t) for t in (ctypes.c_uint64, ctypes.c_float, ctypes.c_uint32))
    qs = np.ascontiguousarray(oracle.gaussian_unit_queries(2, 64), np.float32)
    flat, begin, length = np.arange(4, dtype=np.uint64), np.zeros(2, np.uint64), np.array([4, 5], np.uint64)
    ids, sc, cnt = np.full((2, 3), 55, np.uint64), np.full((2, 3), 5.5, np.float32), np.full(2, 77, np.uint32)
    preds = (_abi.RowPredicate * 2)(_abi.RowPredicate(1, 5, 0, 0, 0), _abi.RowPredicate(0, 0, 0, 0, 1))
    outs = (ids.ctypes.data_as(u64), sc.ctypes.data_as(f32), 3, cnt.ctypes.data_as(u32))
    assert lib.wax_hip_search_batch_predicate(eng._h, None, 0, 64, 10, None, 0, None, None, None, None, None, None, 0, None) == 0   # nq == 0
    rc = lib.wax_hip_search_batch_predicate(eng._h, qs.ctypes.data_as(f32), 2, 64, 10, flat.ctypes.data_as(u64), 4, begin.ctypes.data_as(u64), None,
                                            None, preds, *outs)
    assert rc == _abi.ERR_INVALID_ARGUMENT and _abi.last_error() == "allow_begin and allow_len must both be given or both be null"
    rc = lib.wax_hip_search_batch_predicate(eng._h, qs.ctypes.data_as(f32), 2, 64, 10, flat.ctypes.data_as(u64), 4, begin.ctypes.data_as(u64),
                                            length.ctypes.data_as(u64), None, preds, *outs)
    assert rc == _abi.ERR_INVALID_ARGUMENT and _abi.last_error() == "allow-list range of query 1 leaves the id array"
    rc = lib.wax_hip_search_batch_predicate(eng._h, qs[:, :32].copy().ctypes.data_as(f32), 2, 32, 10, None, 0, None, None, None, preds, *outs)
    assert rc == _abi.ERR_DIM_MISMATCH
    assert (ids == 55).all() and (sc == 5.5).all()
    with pytest.raises(wax.EncodingError):
        eng.searchBatchFiltered(qs, 10, denyFlags=[1, 2, 3])


# ---- 13. sharded ----------------------------------------------------------------------------------------------------------------------

def test_sharded_handle_matches_single_engine(wax):
    n, dims = 30_000, 384
    corpus = corpus_for(0, n, dims, seed=14)
    single, ts, flags = make_engine(wax, 0, dims, corpus, seed=14)
    sharded, _, _ = make_engine(wax, 0, dims, corpus, seed=14, devices=[0, 0, 0])
    assert sharded.getTuning("shards") == 3
    rng = np.random.default_rng(15)
    nq = 24
    queries = oracle.gaussian_unit_queries(nq, dims)
    three = [six_predicates(n)[i] for i in (0, 1, 2)]
    cuts = [None if q % 3 else 0.05 for q in range(nq)]
    for name, lists, preds in (("lists", [random_list(rng, n, [20, 800, 7000, 25000, 0][q % 5]) for q in range(nq)], [(None, 0)] * nq),
                               ("predicates", None, [three[q % 3] for q in range(nq)]),
                               ("both", [None if q % 6 == 5 else random_list(rng, n, [20, 800, 7000, 25000, 0][q % 5]) for q in range(nq)],
                                [three[q % 3] if q % 4 else (None, 0) for q in range(nq)])):
        a = batch(single, queries, 10, preds, lists, cuts)
        b = batch(sharded, queries, 10, preds, lists, cuts)
        assert_rows_equal(b, [(a[0][q, :a[2][q]], a[1][q, :a[2][q]]) for q in range(nq)], f"sharded {name}")
        assert_rows_equal(a, loop(single, queries, 10, preds, lists, cuts), f"single {name}")
    assert sharded.getTuning("predicate_batch_queries") > 0 and sharded.getTuning("filter_batch_fallbacks") == 0
    single.close()
    sharded.close()


# ---- 14. concurrency ------------------------------------------------------------------------------------------------------------------

def test_four_threads_at_once_get_the_serial_answers(wax, store):
    eng, corpus, _, _ = store
    n = len(corpus)
    rng = np.random.default_rng(16)
    nq = 32
    queries = oracle.gaussian_unit_queries(nq, 64)
    three = [six_predicates(n)[i] for i in (0, 1, 2)]
    preds = [three[q % 3] for q in range(nq)]
    lists = [None if q % 2 else random_list(rng, n, [400, 17000][q % 4 // 2]) for q in range(nq)]
    ref = loop(eng, queries, 10, preds, lists)
    results, errors = [None] * 4, []

    def run(i):
        try:
            results[i] = [batch(eng, queries, 10, preds, lists) for _ in range(4)]
        except Exception as exc:   # noqa: BLE001 — reported below, in the test's own thread
            errors.append(exc)
    before = snap(eng)
    threads = [threading.Thread(target=run, args=(i,), daemon=True) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads), "a batched predicate call did not return"
    assert not errors, errors
    for r in results:
        for got in r:
            assert_rows_equal(got, ref, "concurrent")
    assert_pass(eng, before, 16 * nq, 16 * nq, "concurrent")
