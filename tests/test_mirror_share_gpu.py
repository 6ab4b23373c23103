"""Single queries in flight share passes over the bf16 mirror ("mirror_share"): whatever a query rode with, its ids and scores are,
bit for bit, the ones it gets alone ("mirror_share" 0) and the f32 scan's ("scan_mirror" 0).

Every case runs at "scan_mirror" 2 and "mirror_share" 2 (a query is parked until a collect needs it or four are parked), so the
groups are the ones written down here: n submits in a row make passes of 4, 4, ..., n % 4."""
import threading

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

COUNTERS = ("mirror_scans", "mirror_passes", "mirror_shared_passes", "mirror_shared_queries", "mirror_scan_fallbacks",
            "mirror_scan_unavailable")


@pytest.fixture(scope="module")
def wax(hip_lib):
    import wax_amd
    if hip_lib.wax_hip_device_count() == 0:
        pytest.skip("no HIP device on this host: the gpu-marked tests run on the MI355X box (pytest -m gpu)")
    assert hip_lib.wax_hip_available() == 1, "a HIP device is visible but it is not gfx950: the HIP path needs an MI355X"
    return wax_amd


def make_engine(wax, metric, dims, corpus=None, ids=None, **kw):
    eng = wax.HIPVectorEngine(metric=wax.VectorMetric(metric), dimensions=dims, **kw)
    if corpus is not None and len(corpus):
        eng.addBatch(np.arange(len(corpus), dtype=np.uint64) if ids is None else ids, corpus)
    return eng


def corpus_for(metric, n, dims, seed=0):
    x = oracle.gaussian_unit_rows(seed, n, dims)
    if metric == 1:   # dot: rows of different norms
        x = x * np.random.default_rng(seed + 7).uniform(0.5, 2.0, size=(n, 1)).astype(np.float32)
    return np.ascontiguousarray(x, dtype=np.float32)


def counters(eng):
    return {n: eng.getTuning(n) for n in COUNTERS}


def delta(eng, before):
    after = counters(eng)
    return {n: after[n] - before[n] for n in COUNTERS}


def run_group(eng, queries, ks, mirror, share, order=None):
    """Submit every query, then collect (in `order`, default submit order); answers in submit order."""
    eng.setTuning("scan_mirror", mirror)
    eng.setTuning("mirror_share", share)
    tickets = [eng.submit(q, k) for q, k in zip(queries, ks)]
    out = [None] * len(tickets)
    for i in (range(len(tickets)) if order is None else order):
        out[i] = eng.collect(tickets[i], ks[i])
    return out


def same(a, b):
    return all(np.array_equal(x[0], y[0], equal_nan=True) and np.array_equal(x[1], y[1], equal_nan=True) for x, y in zip(a, b)) \
        and len(a) == len(b)


def assert_shared_equals_alone(eng, queries, ks, ctx, order=None):
    """-> the counter deltas of the shared run and of the "mirror_share" 0 run"""
    f32 = run_group(eng, queries, ks, 0, 0)
    c0 = counters(eng)
    alone = run_group(eng, queries, ks, 2, 0)
    d_alone = delta(eng, c0)
    c1 = counters(eng)
    shared = run_group(eng, queries, ks, 2, 2, order)
    d_shared = delta(eng, c1)
    assert same(shared, alone), f"{ctx}: shared pass against one pass per query"
    assert same(shared, f32), f"{ctx}: shared pass against the f32 scan"
    assert d_alone["mirror_shared_passes"] == 0 and d_alone["mirror_passes"] == len(queries)
    assert d_shared["mirror_scans"] == len(queries) and d_shared["mirror_scan_unavailable"] == 0
    assert d_shared["mirror_scan_fallbacks"] == d_alone["mirror_scan_fallbacks"], ctx
    return d_shared, d_alone


@pytest.mark.parametrize("dims", [384, 768])
@pytest.mark.parametrize("metric", [0, 1], ids=["cosine", "dot"])
def test_groups_of_two_to_five_with_mixed_k(wax, metric, dims):
    n = 20005                       # no multiple of the rows per wave iteration (16 at 384-d, 8 at 768-d) nor of the grid's share
    eng = make_engine(wax, metric, dims, corpus_for(metric, n, dims))
    queries = oracle.gaussian_unit_queries(5, dims)
    ks = [10, 1, 32, 10, 1]
    for g in (2, 3, 4, 5):
        d, _ = assert_shared_equals_alone(eng, queries[:g], ks[:g], f"metric {metric} dims {dims} group {g}")
        if g <= 4:
            assert (d["mirror_passes"], d["mirror_shared_passes"], d["mirror_shared_queries"]) == (1, 1, g)
        else:                       # five: a pass of four and a lone one
            assert (d["mirror_passes"], d["mirror_shared_passes"], d["mirror_shared_queries"]) == (2, 1, 4)


def test_store_smaller_than_the_candidate_list_and_row_base(wax):
    dims = 384
    tiny = make_engine(wax, 0, dims, corpus_for(0, 40, dims, seed=2))       # fewer rows than MIRROR_KP = 64 candidates
    queries = oracle.gaussian_unit_queries(4, dims)
    assert_shared_equals_alone(tiny, queries[:3], [10, 32, 1], "40 rows")
    eng = make_engine(wax, 0, dims, corpus_for(0, 9001, dims, seed=3), ids=np.arange(9001, dtype=np.uint64) * 3 + 11)
    eng.setRowBase(123457)
    d, _ = assert_shared_equals_alone(eng, queries, [10, 10, 32, 1], "row_base")
    assert d["mirror_shared_queries"] == 4


def test_one_member_aims_at_duplicates_and_falls_back_alone(wax):
    dims = 384
    queries = list(oracle.gaussian_unit_queries(3, dims))
    dup = corpus_for(0, 10000, dims, seed=41)
    dup[100:200] = queries[1]       # more than 64 exact duplicates of the second query's answer: its certificate cannot hold
    eng = make_engine(wax, 0, dims, dup)
    d, d_alone = assert_shared_equals_alone(eng, queries, [10, 10, 10], "duplicates")
    assert d["mirror_scan_fallbacks"] == 1 and d_alone["mirror_scan_fallbacks"] == 1
    assert (d["mirror_passes"], d["mirror_shared_queries"]) == (1, 3)


@pytest.mark.parametrize("metric", [0, 1], ids=["cosine", "dot"])
def test_zero_and_nan_queries_ride_with_ordinary_ones(wax, metric):
    dims = 384
    eng = make_engine(wax, metric, dims, corpus_for(metric, 7003, dims, seed=43))
    q = oracle.gaussian_unit_queries(2, dims)
    nan_q = q[0].copy()
    nan_q[3] = np.nan
    d, _ = assert_shared_equals_alone(eng, [q[0], np.zeros(dims, np.float32), nan_q, q[1]], [10, 10, 10, 10], f"zero / NaN, metric {metric}")
    assert d["mirror_shared_queries"] == 4


def test_mutations_between_two_groups(wax):
    dims = 384
    eng = make_engine(wax, 0, dims, corpus_for(0, 12000, dims, seed=9))
    queries = oracle.gaussian_unit_queries(3, dims)
    ks = [10, 10, 10]
    assert_shared_equals_alone(eng, queries, ks, "initial")
    eng.addBatch(np.array([7, 11, 900001], dtype=np.uint64), np.stack([queries[0], queries[1] * 1.5, queries[2]]))   # two upserts, one append
    d, _ = assert_shared_equals_alone(eng, queries, ks, "upsert")
    assert d["mirror_shared_queries"] == 3
    eng.setTuning("scan_mirror", 2)
    eng.setTuning("mirror_share", 2)
    assert eng.searchArrays(queries[2], 10)[0][0] in (7, 11, 900001)
    assert eng.removeBatch(np.array([5, 900001, 17, 11999], dtype=np.uint64)) == 4
    assert_shared_equals_alone(eng, queries, ks, "removeBatch")


def test_two_threads_collecting_in_reverse(wax):
    dims, k = 384, 10
    eng = make_engine(wax, 0, dims, corpus_for(0, 15001, dims, seed=13))
    queries = oracle.gaussian_unit_queries(6, dims)
    want = run_group(eng, queries, [k] * 6, 0, 0)
    eng.setTuning("scan_mirror", 2)
    eng.setTuning("mirror_share", 2)
    before = counters(eng)
    got, errors = [None] * 6, []
    submitted = threading.Barrier(2)

    def worker(base):
        try:
            tickets = [eng.submit(queries[base + i], k) for i in range(3)]
            submitted.wait(timeout=60)
            for i in (2, 1, 0):
                got[base + i] = eng.collect(tickets[i], k)
        except Exception as exc:   # noqa: BLE001 — reported by the assertion below
            errors.append(exc)

    threads = [threading.Thread(target=worker, args=(b,)) for b in (0, 3)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert same(got, want)
    d = delta(eng, before)
    assert d["mirror_scans"] == 6 and d["mirror_passes"] == 2 and d["mirror_shared_queries"] == 6   # four, then the two left


def test_closing_with_part_of_a_group_collected_and_with_parked_tickets(wax):
    dims, k = 384, 10
    corpus = corpus_for(0, 8000, dims, seed=17)
    queries = oracle.gaussian_unit_queries(3, dims)
    eng = make_engine(wax, 0, dims, corpus)
    want = run_group(eng, queries[:1], [k], 0, 0)
    eng.setTuning("scan_mirror", 2)
    eng.setTuning("mirror_share", 2)
    tickets = [eng.submit(q, k) for q in queries]
    assert same([eng.collect(tickets[0], k)], want)        # launches all three; two stay uncollected
    eng.close()
    eng = make_engine(wax, 0, dims, corpus)
    eng.setTuning("scan_mirror", 2)
    eng.setTuning("mirror_share", 2)
    for q in queries[:2]:
        eng.submit(q, k)                                     # parked, never launched
    assert eng.getTuning("mirror_passes") == 0
    eng.close()
    again = make_engine(wax, 0, dims, corpus)
    assert same(run_group(again, queries[:1], [k], 2, 2), want)


def test_timed_kernels_stay_one_per_query(wax):
    dims, k = 384, 10
    eng = make_engine(wax, 0, dims, corpus_for(0, 9000, dims, seed=19))
    queries = oracle.gaussian_unit_queries(4, dims)
    want = run_group(eng, queries, [k] * 4, 0, 0)
    eng.setTuning("reset_stats", 1)
    eng.setTuning("time_kernels", 1)
    before = counters(eng)
    got = run_group(eng, queries, [k] * 4, 2, 2)
    d = delta(eng, before)
    eng.setTuning("time_kernels", 0)
    assert same(got, want)
    assert eng.stats().scan_kernels_timed == 4
    assert d["mirror_shared_passes"] == 0 and d["mirror_passes"] == 4 and d["mirror_scans"] == 4


def test_three_shard_handle_answers_like_one_engine(wax):
    dims, k, n = 384, 10, 30000
    corpus = corpus_for(0, n, dims, seed=5)
    many = wax.HIPVectorEngine(dimensions=dims, devices=[0] * 3)
    many.setTuning("shard_min_mb", 0)
    many.addBatch(np.arange(n, dtype=np.uint64), corpus)
    one = make_engine(wax, 0, dims, corpus)
    queries = oracle.gaussian_unit_queries(3, dims)
    want = run_group(one, queries, [k] * 3, 0, 0)
    before = counters(many)
    got = run_group(many, queries, [k] * 3, 2, 2)
    d = delta(many, before)
    assert same(got, want)
    assert d["mirror_scans"] == 9 and d["mirror_passes"] == 3 and d["mirror_shared_queries"] == 9   # one pass of three per shard


def test_lone_blocking_calls_never_share_under_the_default_policy(wax):
    dims, k = 384, 10
    eng = make_engine(wax, 0, dims, corpus_for(0, 6000, dims, seed=23))
    assert eng.getTuning("mirror_share") == 1
    queries = oracle.gaussian_unit_queries(6, dims)
    want = run_group(eng, queries, [k] * 6, 0, 0)
    eng.setTuning("scan_mirror", 2)
    eng.setTuning("mirror_share", 1)
    before = counters(eng)
    got = [eng.searchArrays(q, k) for q in queries]
    d = delta(eng, before)
    assert same(got, want)
    assert d["mirror_shared_passes"] == 0 and d["mirror_passes"] == 6 and d["mirror_scans"] == 6
    with pytest.raises(Exception):
        eng.setTuning("mirror_share", 3)
