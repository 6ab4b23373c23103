"""A caller who pipelines single queries gets full passes over the bf16 mirror ("mirror_fill" 1 under "mirror_share" 1): the bench's
loop (collect the oldest ticket, submit one) parks behind finished uncollected tickets and launches sets of four. Whatever a query
rode with, its ids and scores are, bit for bit, the ones it gets alone ("mirror_share" 0) and the f32 scan's ("scan_mirror" 0).

Stores of 20 005 x 384 (no multiple of the rows per wave iteration) at "scan_mirror" 2, k mixed from 1 / 10 / 32. Where the groups
are pinned, torch.cuda.synchronize() runs before every submit and collect, so that "finished" is a fact and not a race: n queries
at depth d then make one lone pass (the first query finds nothing to wait for), passes of four, and a tail launched by its own
collect."""
import threading

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

COUNTERS = ("mirror_scans", "mirror_passes", "mirror_shared_passes", "mirror_shared_queries", "mirror_scan_fallbacks",
            "mirror_scan_unavailable", "mirror_fill_holds")
N, DIMS, NQ = 20005, 384, 64
KS = [(10, 1, 32)[i % 3] for i in range(NQ)]


@pytest.fixture(scope="module")
def wax(hip_lib):
    import wax_amd
    if hip_lib.wax_hip_device_count() == 0:
        pytest.skip("no HIP device on this host: the gpu-marked tests run on the MI355X box (pytest -m gpu)")
    assert hip_lib.wax_hip_available() == 1, "a HIP device is visible but it is not gfx950: the HIP path needs an MI355X"
    return wax_amd


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x[0], y[0], equal_nan=True) and np.array_equal(x[1], y[1], equal_nan=True)
                                    for x, y in zip(a, b))


def reference(eng, queries, ks):
    """One blocking call per query on the f32 scan and on the mirror without sharing: equal, and what every loop must return."""
    eng.setTuning("scan_mirror", 0)
    eng.setTuning("mirror_share", 0)
    f32 = [eng.searchArrays(q, k) for q, k in zip(queries, ks)]
    eng.setTuning("scan_mirror", 2)
    alone = [eng.searchArrays(q, k) for q, k in zip(queries, ks)]
    assert same(alone, f32), "the mirror alone against the f32 scan"
    return f32


@pytest.fixture(scope="module")
def setup(wax):
    corpus = np.ascontiguousarray(oracle.gaussian_unit_rows(0, N, DIMS), dtype=np.float32)
    eng = wax.HIPVectorEngine(metric=wax.VectorMetric(0), dimensions=DIMS)
    eng.addBatch(np.arange(N, dtype=np.uint64), corpus)
    eng.setTuning("slots", 8)
    queries = oracle.gaussian_unit_queries(NQ, DIMS)
    want = reference(eng, queries, KS)
    yield eng, corpus, queries, want
    eng.close()


def counters(eng):
    return {n: eng.getTuning(n) for n in COUNTERS}


def pipelined(eng, queries, ks, depth, sync=False, fill=1, share=1):
    """bench.py's loop: collect the oldest ticket, submit one. -> (answers in submit order, counter deltas)"""
    import torch
    eng.setTuning("scan_mirror", 2)
    eng.setTuning("mirror_share", share)
    eng.setTuning("mirror_fill", fill)
    torch.cuda.synchronize()
    before = counters(eng)
    pending, out = [], []

    def collect_oldest():
        t, k = pending.pop(0)
        if sync:
            torch.cuda.synchronize()
        out.append(eng.collect(t, k))

    for q, k in zip(queries, ks):
        if len(pending) >= depth:
            collect_oldest()
        if sync:
            torch.cuda.synchronize()
        pending.append((eng.submit(q, k), k))
    while pending:
        collect_oldest()
    after = counters(eng)
    return out, {n: after[n] - before[n] for n in COUNTERS}


def test_the_default_is_on_and_only_zero_or_one_is_accepted(setup):
    eng = setup[0]
    fresh_default = eng.getTuning("mirror_fill")
    with pytest.raises(Exception):
        eng.setTuning("mirror_fill", 2)
    with pytest.raises(Exception):
        eng.setTuning("mirror_fill", -1)
    assert eng.getTuning("mirror_fill") == fresh_default
    assert eng.getTuning("mirror_fill_holds") >= 0


def test_default_of_a_fresh_engine(wax):
    eng = wax.HIPVectorEngine(dimensions=DIMS)
    assert eng.getTuning("mirror_fill") == 1 and eng.getTuning("mirror_share") == 1 and eng.getTuning("mirror_fill_holds") == 0
    eng.close()


def test_depth_four_loop_makes_one_lone_pass_and_then_passes_of_four(setup):
    eng, _, queries, want = setup
    got, d = pipelined(eng, queries[:21], KS[:21], 4, sync=True)
    assert same(got, want[:21])
    assert d["mirror_scans"] == 21 and d["mirror_scan_unavailable"] == 0 and d["mirror_scan_fallbacks"] == 0
    assert (d["mirror_passes"], d["mirror_shared_passes"], d["mirror_shared_queries"]) == (6, 5, 20), d
    assert d["mirror_fill_holds"] > 0
    eager, d0 = pipelined(eng, queries[:21], KS[:21], 4, sync=True, fill=0)
    assert same(eager, want[:21])
    assert d0["mirror_scans"] == 21 and d0["mirror_fill_holds"] == 0


@pytest.mark.parametrize("n,passes", [(5, (2, 1, 4)), (6, (3, 1, 4)), (7, (3, 2, 6))])
def test_loop_lengths_that_do_not_divide(setup, n, passes):
    """n = 6: the sixth query parks behind finished tickets and its own collect launches it alone; n = 7: a tail of two."""
    eng, _, queries, want = setup
    got, d = pipelined(eng, queries[:n], KS[:n], 4, sync=True)
    assert same(got, want[:n])
    assert d["mirror_scans"] == n
    assert (d["mirror_passes"], d["mirror_shared_passes"], d["mirror_shared_queries"]) == passes, d
    raced, d = pipelined(eng, queries[:n], KS[:n], 4)
    assert same(raced, want[:n]) and d["mirror_scans"] == n


def test_depth_eight_loop(setup):
    """24 queries: the first alone, five passes of four, and the three left parked launched by the collect of the first of them."""
    eng, _, queries, want = setup
    got, d = pipelined(eng, queries[:24], KS[:24], 8, sync=True)
    assert same(got, want[:24])
    assert d["mirror_scans"] == 24
    assert (d["mirror_passes"], d["mirror_shared_passes"], d["mirror_shared_queries"]) == (7, 6, 23), d


def test_loop_without_synchronisation(setup):
    eng, _, queries, want = setup
    got, d = pipelined(eng, queries, KS, 4)
    assert same(got, want)
    assert d["mirror_scans"] == NQ and d["mirror_scan_unavailable"] == 0


def test_four_threads_of_blocking_calls_on_one_engine(setup):
    eng, _, queries, want = setup
    eng.setTuning("scan_mirror", 2)
    eng.setTuning("mirror_share", 1)
    eng.setTuning("mirror_fill", 1)
    before = counters(eng)
    got, errors = [None] * 24, []

    def worker(base):
        try:
            for i in range(base, base + 6):
                got[i] = eng.searchArrays(queries[i], KS[i])
        except Exception as exc:   # noqa: BLE001 — reported by the assertion below
            errors.append(exc)

    threads = [threading.Thread(target=worker, args=(b,), daemon=True) for b in (0, 6, 12, 18)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=60)
    assert not any(t.is_alive() for t in threads), "a ticket was left parked: a blocking call did not return"
    assert not errors, errors
    assert same(got, want[:24])
    assert eng.getTuning("mirror_scans") - before["mirror_scans"] == 24


def test_three_shard_handle_answers_like_one_engine(wax, setup):
    _, corpus, queries, want = setup
    many = wax.HIPVectorEngine(dimensions=DIMS, devices=[0] * 3)
    many.setTuning("shard_min_mb", 0)
    many.addBatch(np.arange(N, dtype=np.uint64), corpus)
    assert many.getTuning("mirror_fill") == 1
    got, d = pipelined(many, queries[:13], KS[:13], 4)
    assert same(got, want[:13])
    assert d["mirror_scans"] == 39 and d["mirror_scan_unavailable"] == 0   # every query on each of the three shards
    synced, d = pipelined(many, queries[:13], KS[:13], 4, sync=True)
    assert same(synced, want[:13])
    assert (d["mirror_passes"], d["mirror_shared_passes"], d["mirror_shared_queries"]) == (12, 9, 36), d   # 1 + 3 passes of four per shard
    many.close()


def test_one_member_of_a_full_pass_aims_at_duplicates_and_falls_back_alone(wax, setup):
    _, corpus, queries, _ = setup
    dup = corpus.copy()
    dup[100:200] = queries[2]      # more than 64 exact duplicates of the third query's answer: its certificate cannot hold
    eng = wax.HIPVectorEngine(metric=wax.VectorMetric(0), dimensions=DIMS)
    eng.addBatch(np.arange(N, dtype=np.uint64), dup)
    want = reference(eng, queries[:9], KS[:9])
    f0 = eng.getTuning("mirror_scan_fallbacks")
    got, d = pipelined(eng, queries[:9], KS[:9], 4, sync=True)     # the third query rides in the first pass of four
    assert same(got, want)
    assert (d["mirror_passes"], d["mirror_shared_passes"], d["mirror_shared_queries"]) == (3, 2, 8), d
    assert d["mirror_scan_fallbacks"] == 1 and f0 == 1
    eng.close()


def test_timed_kernels_make_no_shared_pass_and_hold_nothing(setup):
    eng, _, queries, want = setup
    eng.setTuning("time_kernels", 1)
    try:
        got, d = pipelined(eng, queries[:13], KS[:13], 4)
        synced, ds = pipelined(eng, queries[:13], KS[:13], 4, sync=True)
    finally:
        eng.setTuning("time_kernels", 0)
    assert same(got, want[:13]) and same(synced, want[:13])
    for c in (d, ds):
        assert c["mirror_shared_passes"] == 0 and c["mirror_passes"] == 13 and c["mirror_scans"] == 13 and c["mirror_fill_holds"] == 0
