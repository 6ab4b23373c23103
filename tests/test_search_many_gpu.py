"""One query each against many small stores in one pass (wax_hip_search_many / wax_amd.searchMany): row i must equal what
engines[i].search(queries[i], topK) returns — ids, scores and counts bit for bit — whether the pooled launch or the single-query
search answered the pair, and the two read-only counters must show which did."""
import ctypes
import threading

import numpy as np
import pytest

import oracle
from helpers import assert_parity

pytestmark = pytest.mark.gpu

GROUP = {64: 16, 384: 32, 768: 64}     # row_math.h's lane-shape table at the dims under test
N_ENGINES = 40
KS = (1, 10, 60, 61, 192, 193, 5000)   # 61: 256-slot lists where LDS allows; 193 and 5000 (> every store's rows): always the loop


@pytest.fixture(scope="module")
def wax(hip_lib):
    import wax_amd
    if hip_lib.wax_hip_device_count() == 0:
        pytest.skip("no HIP device on this host: the gpu-marked tests run on the MI355X box (pytest -m gpu)")
    assert hip_lib.wax_hip_available() == 1, "a HIP device is visible but it is not gfx950: the HIP path needs an MI355X"
    return wax_amd


def rpc(dims):
    """rows a wave consumes per chunk"""
    return (64 // GROUP[dims]) * 4


def pooled_shape(dims, k):
    """scan_multi_group(dims, k) != 0: k <= 192 and the 16 queries with their four wave lists (64 slots while k + 4 <= 64, else 256)
    fit the 160 KB of LDS (multiscan.hip: scan_multi_lds_bytes)."""
    if k < 1 or k > 192:
        return False
    cap = 64 if k + 4 <= 64 else 256
    return 16 * dims * 4 + 4 * 16 * cap * 8 + 4 * 16 * 16 + 16 * 4 + 16 * 4 * 4 + 16 <= 160 * 1024


def corpus_for(metric, n, dims, seed):
    x = oracle.gaussian_unit_rows(seed * 100003, n, dims)
    if metric == 1:   # dot: rows of different norms
        x = x * np.random.default_rng(seed + 7).uniform(0.5, 2.0, size=(n, 1)).astype(np.float32)
    return np.ascontiguousarray(x, dtype=np.float32)


def make_engine(wax, metric, dims, corpus=None, ids=None, **kw):
    eng = wax.HIPVectorEngine(metric=wax.VectorMetric(metric), dimensions=dims, **kw)
    if corpus is not None and len(corpus):
        eng.addBatch(ids, corpus)
    return eng


def loop(engines, queries, k):
    return [engines[i].searchArrays(queries[i], k) for i in range(len(engines))]


def assert_rows_equal(many, ref, ctx):
    ids, scores, counts = many
    for i, (ri, rs) in enumerate(ref):
        n = int(counts[i])
        assert n == len(ri), f"{ctx}: pair {i} count {n} != {len(ri)}"
        assert np.array_equal(ids[i, :n], ri), f"{ctx}: pair {i} ids"
        assert np.array_equal(scores[i, :n], rs), f"{ctx}: pair {i} scores"


def counters(engines):
    distinct = {id(e): e for e in engines}.values()
    return {id(e): (e.getTuning("search_many_pooled"), e.getTuning("search_many_looped")) for e in distinct}


def assert_route(engines, before, pooled, ctx):
    """every pair went the expected way: per distinct engine, the counter of that route grew by its pairs and the other stood still"""
    after = counters(engines)
    for e in {id(e): e for e in engines}.values():
        pairs = sum(1 for x in engines if x is e)
        dp, dl = after[id(e)][0] - before[id(e)][0], after[id(e)][1] - before[id(e)][1]
        want = pooled(e) if callable(pooled) else pooled
        assert (dp, dl) == ((pairs, 0) if want else (0, pairs)), f"{ctx}: engine of {e.count} rows listed {pairs}x: pooled +{dp}, looped +{dl}"


class Stores:
    """About 40 engines of one (dims, metric), sizes around the chunk boundaries, overlapping id spaces; a list of 100 pairs."""

    def __init__(self, wax, dims, metric):
        r = rpc(dims)
        sizes = [0, 1, r - 1, r, r + 1, 16 * r + 3, 3000]
        rng = np.random.default_rng(dims * 10 + metric)
        self.engines, self.corpora, self.ids = [], [], []
        for j in range(N_ENGINES):
            n = sizes[j % len(sizes)]
            c = corpus_for(metric, n, dims, seed=j + 1)
            if j == 6:   # the first 3 000-row store: exactly duplicated rows (the tie order is ascending ROW, not ascending id)
                c[100:110] = c[50]
                c[2990:2995] = c[50]
            ids = (1000 * j + rng.permutation(n)).astype(np.uint64)   # engine j's ids overlap its neighbours'; row order != id order
            self.engines.append(make_engine(wax, metric, dims, c, ids))
            self.corpora.append(c)
            self.ids.append(ids)
        order = [5] * 17 + [6] * 33 + [0] * 2           # 17 = two groups, 33 = three, the empty engine twice
        rest = [j for j in range(N_ENGINES) if j not in (0, 5, 6)]
        order += rest + rest[:100 - len(order) - len(rest)]
        assert len(order) == 100
        self.order = [int(j) for j in rng.permutation(order)]
        self.queries = oracle.gaussian_unit_queries(100, dims, seed=dims + metric).copy()
        for i, j in enumerate(self.order):
            if j == 6 and i % 2 == 0:   # half of the duplicated store's queries sit on its duplicated row: the ties are the top hits
                self.queries[i] = self.corpora[6][50] + 1e-3 * self.queries[i]
        self.pairs = [self.engines[j] for j in self.order]
        self.ref = {}

    def reference(self, k):
        if k not in self.ref:
            self.ref[k] = loop(self.pairs, self.queries, k)
        return self.ref[k]

    def close(self):
        for e in self.engines:
            e.close()


@pytest.fixture(scope="module")
def stores(wax):
    made = {}

    def get(dims, metric):
        if (dims, metric) not in made:
            made[(dims, metric)] = Stores(wax, dims, metric)
        return made[(dims, metric)]
    yield get
    for s in made.values():
        s.close()


@pytest.mark.parametrize("metric", [0, 1, 2], ids=["cosine", "dot", "l2"])
@pytest.mark.parametrize("dims", [64, 384, 768])
def test_many_equals_loop(wax, stores, dims, metric):
    s = stores(dims, metric)
    for k in KS:
        ref = s.reference(k)
        before = counters(s.pairs)
        got = wax.searchMany(s.pairs, s.queries, k)
        assert_rows_equal(got, ref, f"dims {dims} metric {metric} k {k}")
        assert_route(s.pairs, before, pooled_shape(dims, k), f"dims {dims} metric {metric} k {k}")
    assert pooled_shape(dims, 60) and not pooled_shape(dims, 193)
    assert pooled_shape(dims, 61) == (dims < 768)      # 256-slot lists beside sixteen 768-d queries do not fit LDS


def test_ties_come_in_ascending_row_order(wax, stores):
    s = stores(384, 0)
    e, ids = s.engines[6], s.ids[6]
    q = np.stack([s.corpora[6][50]] * 2)
    got_ids, _, counts = wax.searchMany([e, e], q, 16)
    want = [int(ids[r]) for r in [50] + list(range(100, 110)) + list(range(2990, 2995))]
    assert counts.tolist() == [16, 16] and got_ids[0].tolist() == want and got_ids[1].tolist() == want


def test_other_dims_take_the_loop(wax):
    dims = 100
    engines = [make_engine(wax, 0, dims, corpus_for(0, n, dims, seed=n), (1000 * j + np.arange(n)).astype(np.uint64))
               for j, n in enumerate([0, 7, 300])]
    pairs = [engines[j] for j in (2, 0, 1, 2, 1)]
    queries = oracle.gaussian_unit_queries(len(pairs), dims)
    before = counters(pairs)
    assert_rows_equal(wax.searchMany(pairs, queries, 10), loop(pairs, queries, 10), "dims 100")
    assert_route(pairs, before, False, "dims 100")
    for e in engines:
        e.close()


def test_switch_and_row_limit_route_per_engine(wax, stores):
    s = stores(384, 0)
    ref = s.reference(10)
    big = lambda e: e.count > 1000
    try:
        for e in s.engines:
            e.setTuning("search_many_max_rows", 1000)
        before = counters(s.pairs)
        assert_rows_equal(wax.searchMany(s.pairs, s.queries, 10), ref, "max_rows 1000")
        assert any(big(e) for e in s.pairs) and not all(big(e) for e in s.pairs)
        assert_route(s.pairs, before, lambda e: not big(e), "max_rows 1000")      # looped and pooled pairs in ONE call
    finally:
        for e in s.engines:
            e.setTuning("search_many_max_rows", 262144)
    off = s.engines[5]
    try:
        off.setTuning("search_many", 0)
        before = counters(s.pairs)
        assert_rows_equal(wax.searchMany(s.pairs, s.queries, 10), ref, "search_many 0 on one engine")
        assert_route(s.pairs, before, lambda e: e is not off, "search_many 0 on one engine")
    finally:
        off.setTuning("search_many", 1)
    try:
        for e in s.engines:
            e.setTuning("search_many", 0)
        before = counters(s.pairs)
        assert_rows_equal(wax.searchMany(s.pairs, s.queries, 10), ref, "search_many 0")
        assert_route(s.pairs, before, False, "search_many 0")
    finally:
        for e in s.engines:
            e.setTuning("search_many", 1)


def test_accounting_charges_each_engine_what_was_read(wax, stores):
    s = stores(384, 0)
    seen = {}
    for e in s.pairs:
        seen.setdefault(id(e), [e, 0])[1] += 1
    before = {i: (e.stats(), n) for i, (e, n) in seen.items()}
    wax.searchMany(s.pairs, s.queries, 10)
    for i, (e, n) in seen.items():
        st0, st1 = before[i][0], e.stats()
        groups = (n + 15) // 16 if e.count else 0
        assert st1.searches - st0.searches == n
        assert st1.rows_scanned - st0.rows_scanned == e.count * groups          # the store once per group of 16 queries
        assert st1.bytes_scanned - st0.bytes_scanned == e.count * groups * 384 * 4


def test_a_row_added_just_before_the_call_is_seen(wax):
    dims = 384
    engines = [make_engine(wax, 0, dims, corpus_for(0, 200, dims, seed=40 + j), (1000 * j + np.arange(200)).astype(np.uint64))
               for j in range(3)]
    queries = oracle.gaussian_unit_queries(3, dims, seed=5).copy()
    engines[1].add(999_999, queries[1])              # staged on the host until the next reader flushes it
    ids, scores, counts = wax.searchMany(engines, queries, 5)
    assert ids[1, 0] == 999_999 and abs(float(scores[1, 0]) - 1.0) < 1e-5
    assert_rows_equal((ids, scores, counts), loop(engines, queries, 5), "staged append")
    for e in engines:
        e.close()


def raw_many(hip_lib, engines, queries, k, stride):
    """the C call itself, outputs pre-filled with 7: (rc, message, ids, scores, counts)"""
    from wax_amd import _abi
    f32, u32, u64 = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
    n = len(engines)
    handles = (ctypes.c_void_p * n)(*[e._h.value for e in engines])
    q = np.ascontiguousarray(queries, dtype=np.float32)
    ids, scores, counts = np.full((n, stride), 7, np.uint64), np.full((n, stride), 7, np.float32), np.full(n, 7, np.uint32)
    rc = hip_lib.wax_hip_search_many(handles, q.ctypes.data_as(f32), n, q.shape[1], k, ids.ctypes.data_as(u64), scores.ctypes.data_as(f32),
                                     stride, counts.ctypes.data_as(u32))
    return rc, _abi.last_error(), ids, scores, counts


def test_refusals_name_the_pair_and_touch_nothing(wax, hip_lib):
    from wax_amd import _abi
    dims = 64
    c = corpus_for(0, 50, dims, seed=3)
    ids = np.arange(50, dtype=np.uint64)
    a, b = make_engine(wax, 0, dims, c, ids), make_engine(wax, 0, dims, c, ids)
    other_dims = make_engine(wax, 0, 128, corpus_for(0, 50, 128, seed=3), ids)
    other_metric = make_engine(wax, 2, dims, c, ids)
    sharded = make_engine(wax, 0, dims, c, ids, devices=[0, 0])
    q = oracle.gaussian_unit_queries(3, dims)
    cases = [([a, b, other_dims], _abi.ERR_DIM_MISMATCH, "pair 2"),
             ([a, other_metric, b], _abi.ERR_INVALID_ARGUMENT, "pair 1"),
             ([a, b, sharded], _abi.ERR_INVALID_ARGUMENT, "pair 2")]
    for engines, code, who in cases:
        before = counters([a, b])
        rc, msg, ids_o, scores_o, counts_o = raw_many(hip_lib, engines, q, 10, 10)
        assert rc == code and who in msg, (rc, msg)
        assert (ids_o == 7).all() and (scores_o == 7).all() and (counts_o == 7).all(), msg
        assert counters([a, b]) == before
    # the dimension refusal carries wax_hip_search's message
    with pytest.raises(Exception) as single:
        other_dims.searchArrays(q[0], 10)
    assert str(single.value) in raw_many(hip_lib, [a, b, other_dims], q, 10, 10)[1]
    with pytest.raises(Exception):
        wax.searchMany([a, b, sharded], q, 10)
    for e in (a, b, other_dims, other_metric, sharded):
        e.close()


def test_opposite_orders_and_a_writer_do_not_deadlock(wax):
    """A host deadlock check: two readers list the same 8 engines in opposite orders while a writer upserts rows with their own
    vectors (exclusive lock, one engine at a time), so no answer can change."""
    dims, n, calls = 64, 200, 200
    corpora = [corpus_for(0, n, dims, seed=70 + j) for j in range(8)]
    engines = [make_engine(wax, 0, dims, corpora[j], (1000 * j + np.arange(n)).astype(np.uint64)) for j in range(8)]
    queries = oracle.gaussian_unit_queries(8, dims, seed=9)
    ref = loop(engines, queries, 10)
    rev = list(reversed(range(8)))
    errors = []

    def reader(order):
        try:
            pairs, qs, want = [engines[j] for j in order], queries[order], [ref[j] for j in order]
            for _ in range(calls):
                assert_rows_equal(wax.searchMany(pairs, qs, 10), want, f"order {order[0]}..")
        except BaseException as exc:   # noqa: BLE001 — reported by the main thread
            errors.append(exc)

    def writer():
        try:
            for i in range(calls):
                j, r = i % 8, (i * 37) % n
                engines[j].add(1000 * j + r, corpora[j][r])
        except BaseException as exc:   # noqa: BLE001
            errors.append(exc)

    threads = [threading.Thread(target=reader, args=(list(range(8)),)), threading.Thread(target=reader, args=(rev,)),
               threading.Thread(target=writer)]
    for t in threads:
        t.daemon = True
        t.start()
    for t in threads:
        t.join(timeout=60)
    assert not any(t.is_alive() for t in threads), "a thread is still running after 60 s: deadlock"
    assert not errors, errors[0]
    assert_rows_equal(wax.searchMany(engines, queries, 10), ref, "after the writer")
    for e in engines:
        e.close()


def test_against_the_oracle(wax):
    dims, n, k = 384, 500, 10
    corpora = [corpus_for(0, n, dims, seed=90 + j) for j in range(5)]
    rng = np.random.default_rng(4)
    ids = [(1000 * j + rng.permutation(n)).astype(np.uint64) for j in range(5)]
    engines = [make_engine(wax, 0, dims, corpora[j], ids[j]) for j in range(5)]
    queries = oracle.gaussian_unit_queries(5, dims, seed=11)
    before = counters(engines)
    got_ids, got_scores, counts = wax.searchMany(engines, queries, k)
    assert_route(engines, before, True, "oracle case")
    for j in range(5):
        ei, es, _, _ = oracle.search(0, corpora[j], ids[j], queries[j], k)
        _, es_all, _, _ = oracle.search(0, corpora[j], ids[j], queries[j], 2 * k)
        c = int(counts[j])
        assert c == len(ei)
        assert_parity(got_ids[j, :c], got_scores[j, :c], ei, es, all_exp_scores=es_all, ctx=f"engine {j}")
    for e in engines:
        e.close()
