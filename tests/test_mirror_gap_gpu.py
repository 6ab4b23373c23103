"""The finish and host leg between shared mirror passes: the finish's selection of its 64 approximate candidates (the lists' prefixes
under a bound from their heads, the k-way merge where they overflow its buffer) and the members' queries uploaded by one launch in
front of the group scan. Mirror tickets complete through their events at either "done_flag" setting (a finish that published the
slot's completion word was measured and dropped, profiles/r24): both settings are held to the same answers and counters.

Nothing here may change an answer: every query's ids and scores are, with array_equal, the same engine's at "scan_mirror" 0 (the f32
scan), whichever way the selection went and whatever the query rode with. Stores of 20 005 x 384 (no multiple of 16) at
"scan_mirror" 2, on the 8-bit code mirror (k = 1, 10, 16) and on bf16 (k = 32). Where counters are compared,
torch.cuda.synchronize() runs before every submit and collect, so that "finished" is a fact and not a race."""
import threading

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

COUNTERS = ("mirror_scans", "mirror_passes", "mirror_shared_passes", "mirror_shared_queries", "mirror_scan_fallbacks",
            "mirror_scan_unavailable", "mirror8_passes", "mirror8_fallbacks", "done_flag_waits")
N, DIMS, NQ = 20005, 384, 64
KS = {8: [(10, 1, 16)[i % 3] for i in range(NQ)], 16: [32] * NQ}
BITS = (8, 16)


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


def counters(eng):
    return {n: eng.getTuning(n) for n in COUNTERS}


def delta(eng, before):
    after = counters(eng)
    return {n: after[n] - before[n] for n in COUNTERS}


def engine(wax, rows):
    eng = wax.HIPVectorEngine(metric=wax.VectorMetric(0), dimensions=DIMS)
    eng.addBatch(np.arange(len(rows), dtype=np.uint64), np.ascontiguousarray(rows, dtype=np.float32))
    eng.setTuning("slots", 8)
    return eng


def truth(eng, queries, ks):
    """the f32 scan, one blocking call per query"""
    eng.setTuning("scan_mirror", 0)
    out = [eng.searchArrays(q, k) for q, k in zip(queries, ks)]
    eng.setTuning("scan_mirror", 2)
    return out


def on_mirror(eng, bits, share=1, done_flag=1):
    """route single queries to the mirror of `bits`; the code mirror is built by the third query that wants it: ask four times"""
    eng.setTuning("scan_mirror", 2)
    eng.setTuning("mirror_bits", bits)
    eng.setTuning("mirror_share", 0)
    eng.setTuning("done_flag", done_flag)
    probe = oracle.gaussian_unit_queries(1, DIMS)[0]
    for _ in range(4):
        eng.searchArrays(probe, 1)
    eng.setTuning("mirror_share", share)
    eng.setTuning("mirror_fill", 1)


def pipelined(eng, queries, ks, depth, sync):
    """bench.py's loop: collect the oldest ticket, submit one. -> (answers in submit order, counter deltas)"""
    import torch
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
    return out, delta(eng, before)


@pytest.fixture(scope="module")
def setup(wax):
    corpus = np.ascontiguousarray(oracle.gaussian_unit_rows(0, N, DIMS), dtype=np.float32)
    eng = engine(wax, corpus)
    queries = oracle.gaussian_unit_queries(NQ, DIMS)
    want = {bits: truth(eng, queries, KS[bits]) for bits in BITS}
    yield eng, corpus, queries, want
    eng.close()


# ---- the depth-four loop at both "done_flag" settings ----

@pytest.mark.parametrize("bits", BITS)
def test_depth_four_loop_is_the_f32_scan_at_both_done_flag_settings(setup, bits):
    eng, _, queries, want = setup
    ks = KS[bits]
    seen = {}
    for flag in (1, 0):
        on_mirror(eng, bits, done_flag=flag)
        got, d = pipelined(eng, queries, ks, 4, sync=True)
        assert same(got, want[bits]), (bits, flag)
        raced, dr = pipelined(eng, queries, ks, 4, sync=False)
        assert same(raced, want[bits]), (bits, flag)
        assert dr["mirror_scans"] == NQ and dr["mirror_scan_fallbacks"] == 0 and dr["done_flag_waits"] == 0
        seen[flag] = d
    eng.setTuning("done_flag", 1)
    d = seen[1]
    assert d == seen[0], seen
    assert d["mirror_scans"] == NQ and d["mirror_scan_fallbacks"] == 0 and d["mirror_scan_unavailable"] == 0 and d["mirror8_fallbacks"] == 0
    # the first query alone, fifteen passes of four, the last three launched by the collect of the first of them
    assert (d["mirror_passes"], d["mirror_shared_passes"], d["mirror_shared_queries"]) == (17, 16, 63), d
    assert d["mirror8_passes"] == (17 if bits == 8 else 0)
    assert d["done_flag_waits"] == 0, "a mirror ticket is not a counted flag wait"


def test_f32_tickets_still_count_their_flag_waits(setup):
    eng, _, queries, want = setup
    eng.setTuning("done_flag", 1)
    eng.setTuning("scan_mirror", 0)
    before = eng.getTuning("done_flag_waits")
    got = eng.searchArrays(queries[0], 10)
    eng.setTuning("scan_mirror", 2)
    assert same([got], want[8][:1])
    assert eng.getTuning("done_flag_waits") == before + 1


# ---- the selection itself: both ways on the same lists (wax_hip_mirror_select_probe) ----
# Keys are (word : row) like the scan's; a list is ascending and KEY_PAD-padded. The model of the bound is topk.h's gather_select: thread
# (wave w, lane l) owns lists 4 l + w (+ 256), a lane's value is the smaller word of its heads, a wave takes its 16th smallest, the
# bound is the largest of the four; the gather answers when at most 128 keys have a word <= the bound.

KP, CAP, PAD = 64, 128, (1 << 63) - 1


def make_lists(per_list):
    """per_list: one array of (word, row) pairs per list -> [lists][64] int64, sorted, padded"""
    out = np.full((len(per_list), KP), PAD, dtype=np.int64)
    for i, pairs in enumerate(per_list):
        keys = np.sort(np.array([(int(w) << 32) | int(r) for w, r in pairs], dtype=np.int64))[:KP]
        out[i, :len(keys)] = keys
    return out


def keys_under_bound(lists):
    x = np.full((4, 64), (1 << 31) - 1, dtype=np.int64)
    for i, head in enumerate(lists[:, 0] >> 32):
        w, lane = i % 4, (i % 256) // 4
        x[w, lane] = min(x[w, lane], head)
    bound = max(np.sort(x[w])[15] for w in range(4))
    return int(np.sum((lists != PAD) & ((lists >> 32) <= bound)))


def probe(hip_lib, lists):
    import ctypes
    lists = np.ascontiguousarray(lists, dtype=np.int64)
    sel, mer, took = np.zeros(KP, np.int64), np.zeros(KP, np.int64), ctypes.c_int32(-1)
    p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))   # noqa: E731
    rc = hip_lib.wax_hip_mirror_select_probe(p(lists), len(lists), p(sel), p(mer), ctypes.byref(took))
    assert rc == 0, rc
    live = np.sort(lists[lists != PAD])[:KP]
    want = np.concatenate([live, np.full(KP - len(live), PAD, dtype=np.int64)])
    assert np.array_equal(mer, want), "the k-way merge against a host sort"
    assert np.array_equal(sel, mer), "the finish's selection against the k-way merge"
    assert took.value == (1 if keys_under_bound(lists) <= CAP else 0)
    return took.value


def random_lists(seed, n_lists, rows_per_list=64):
    rng = np.random.default_rng(seed)
    words = rng.integers(1 << 20, 1 << 30, size=(n_lists, rows_per_list))
    return make_lists([[(w, i * rows_per_list + j) for j, w in enumerate(ws)] for i, ws in enumerate(words)])


@pytest.mark.parametrize("n_lists", [505, 313, 256, 257, 100, 64, 5, 1])
def test_selection_on_random_lists(wax, hip_lib, n_lists):
    took = probe(hip_lib, random_lists(n_lists, n_lists))
    if n_lists in (505, 313):
        assert took == 1, "uniform keys over hundreds of lists: the gather's side"


def test_selection_with_all_the_best_in_two_lists(wax, hip_lib):
    lists = random_lists(3, 505)
    lists[7] = make_lists([[(5, r) for r in range(64)]])[0]
    lists[300] = make_lists([[(6, 1000 + r) for r in range(64)]])[0]
    assert probe(hip_lib, lists) == 0


def test_selection_with_equal_words_everywhere(wax, hip_lib):
    assert probe(hip_lib, make_lists([[(9, i * 64 + j) for j in range(64)] for i in range(505)])) == 0


@pytest.mark.parametrize("n_lists,per", [(3, 10), (1, 63), (2, 64), (3, 64), (40, 1)])
def test_selection_with_few_keys(wax, hip_lib, n_lists, per):
    """fewer than 64 keys in all (KEY_PAD-padded answer), two full lists (128 keys: gathered), three (192: merged)"""
    rng = np.random.default_rng(per)
    took = probe(hip_lib, make_lists([[(int(w), i * 64 + j) for j, w in enumerate(rng.integers(1, 1000, size=per))] for i in range(n_lists)]))
    assert took == (1 if n_lists * per <= CAP else 0)


@pytest.mark.parametrize("under", [127, 128, 129])
def test_selection_at_the_edge_of_the_gather_buffer(wax, hip_lib, under):
    """256 lists; lists 0 .. 63 (sixteen lanes of each wave) have heads of word 10, the others of word 1 000: the bound is 10. List 0
    holds 64 keys of word 10, which with the 63 other heads makes 127 under the bound; lists 1 and 2 add one each."""
    per = [[(10, i * 64)] + [(2000 + j, i * 64 + j) for j in range(1, 64)] if i < 64 else [(1000 + j, i * 64 + j) for j in range(64)] for i in range(256)]
    per[0] = [(10, j) for j in range(64)]
    for extra in range(under - 127):
        per[1 + extra][1] = (10, (1 + extra) * 64 + 1)
    lists = make_lists(per)
    assert keys_under_bound(lists) == under
    assert probe(hip_lib, lists) == (1 if under <= CAP else 0)


# ---- the selection's edges, end to end ----

def run_edge(eng, bits, queries, ks):
    """every query alone and in one set of up to four -> counter deltas of the lone round"""
    want = truth(eng, queries, ks)
    on_mirror(eng, bits, share=0)
    before = counters(eng)
    alone = [eng.searchArrays(q, k) for q, k in zip(queries, ks)]
    d = delta(eng, before)
    assert same(alone, want), bits
    eng.setTuning("mirror_share", 2)
    tickets = [(eng.submit(q, k), k) for q, k in zip(queries[:4], ks[:4])]
    shared = [eng.collect(t, k) for t, k in tickets]
    assert same(shared, want[:4]), bits
    return d


def edge_ks(bits, n):
    return [(10, 1, 16)[i % 3] if bits == 8 else 32 for i in range(n)]


@pytest.mark.parametrize("bits", BITS)
def test_all_the_best_rows_in_two_workgroups_lists(wax, setup, bits):
    """Rows 0 .. 79 are near-copies of the query at 80 distinct scores: the 64 best sit in the lists of the first two workgroups, on the
    side of the selection where more keys lie under the heads' bound than the gather buffer holds (which way a finish went is not
    visible from here: the probe tests below pin the two ways to each other)."""
    _, corpus, queries, _ = setup
    q = np.asarray(queries[5], dtype=np.float64)
    u = np.asarray(queries[6], dtype=np.float64)
    u -= (u @ q) * q
    u /= np.linalg.norm(u)
    rows = corpus.copy()
    theta = 0.01 * (1 + np.arange(80))
    rows[:80] = (np.cos(theta)[:, None] * q + np.sin(theta)[:, None] * u).astype(np.float32)
    assert len(np.unique(rows[:80].astype(np.float64) @ q)) == 80
    eng = engine(wax, rows)
    qs = [queries[5], queries[7], queries[5], queries[8]]
    d = run_edge(eng, bits, qs, edge_ks(bits, 4))
    assert d["mirror_scans"] == 4 and d["mirror_scan_unavailable"] == 0
    eng.close()


@pytest.mark.parametrize("bits", BITS)
def test_duplicates_are_refused_and_answered_exactly(wax, setup, bits):
    _, corpus, queries, _ = setup
    rows = corpus.copy()
    rows[3000:3000 + 2048] = corpus[17]
    eng = engine(wax, rows)
    d = run_edge(eng, bits, [corpus[17], queries[1]], edge_ks(bits, 2))
    assert d["mirror_scans"] == 2
    assert d["mirror_scan_fallbacks"] == 1, "2 048 equal distances around the 64th candidate: the certificate must refuse"
    eng.close()


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("n", [50, 64, 200])
def test_stores_of_a_few_rows(wax, setup, bits, n):
    """fewer rows than candidates (KEY_PAD-padded: never certified, answered exactly all the same), exactly as many, and a few lists"""
    _, corpus, queries, _ = setup
    eng = engine(wax, corpus[:n])
    d = run_edge(eng, bits, list(queries[:4]), edge_ks(bits, 4))
    assert d["mirror_scans"] == 4, "forced with \"scan_mirror\" 2 the route takes a store of any size"
    if n < 64:
        assert d["mirror_scan_fallbacks"] == 4
    eng.close()


@pytest.mark.parametrize("bits", BITS)
def test_nan_and_zero_queries(setup, bits):
    eng, _, queries, _ = setup
    bad = np.array(queries[3], dtype=np.float32)
    bad[7] = np.nan
    zero = np.zeros(DIMS, dtype=np.float32)
    d = run_edge(eng, bits, [bad, zero, queries[4]], edge_ks(bits, 3))
    assert d["mirror_scans"] == 3


# ---- the queries of a set ----

@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("n", [2, 3, 4])
def test_sets_collected_in_reverse_order(setup, bits, n):
    eng, _, queries, want = setup
    on_mirror(eng, bits, share=2)
    before = counters(eng)
    tickets = [(eng.submit(queries[i], KS[bits][i]), KS[bits][i]) for i in range(n)]
    got = [eng.collect(t, k) for t, k in reversed(tickets)][::-1]
    d = delta(eng, before)
    assert same(got, want[bits][:n])
    assert (d["mirror_passes"], d["mirror_shared_passes"], d["mirror_shared_queries"], d["mirror_scan_fallbacks"]) == (1, 1, n, 0), d


@pytest.mark.parametrize("bits", [0, 8])
def test_a_member_of_k_32_takes_its_set_to_bf16(setup, bits):
    eng, _, queries, _ = setup
    ks = [10, 32, 1, 16]
    expect = truth(eng, queries[:4], ks)
    on_mirror(eng, bits, share=2)
    before = counters(eng)
    tickets = [(eng.submit(queries[i], k), k) for i, k in enumerate(ks)]
    got = [eng.collect(t, k) for t, k in tickets]
    d = delta(eng, before)
    assert same(got, expect)
    assert (d["mirror_passes"], d["mirror_shared_passes"], d["mirror_shared_queries"], d["mirror8_passes"]) == (1, 1, 4, 0), d


@pytest.mark.parametrize("bits", BITS)
def test_a_parked_ticket_collected_before_its_set_fills_launches_alone(setup, bits):
    eng, _, queries, want = setup
    on_mirror(eng, bits, share=2)
    before = counters(eng)
    t = eng.submit(queries[9], KS[bits][9])
    got = eng.collect(t, KS[bits][9])
    d = delta(eng, before)
    assert same([got], want[bits][9:10])
    assert (d["mirror_scans"], d["mirror_passes"], d["mirror_shared_passes"]) == (1, 1, 0), d


@pytest.mark.parametrize("bits", BITS)
def test_four_threads_of_blocking_calls_on_one_engine(setup, bits):
    eng, _, queries, want = setup
    on_mirror(eng, bits, share=1)
    before = counters(eng)
    got, errors = [None] * 24, []

    def worker(base):
        try:
            for i in range(base, base + 6):
                got[i] = eng.searchArrays(queries[i], KS[bits][i])
        except Exception as exc:   # noqa: BLE001 — reported by the assertion below
            errors.append(exc)

    threads = [threading.Thread(target=worker, args=(b,), daemon=True) for b in (0, 6, 12, 18)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=60)
    assert not any(t.is_alive() for t in threads), "a ticket was left parked: a blocking call did not return"
    assert not errors, errors
    assert same(got, want[bits][:24])
    assert delta(eng, before)["mirror_scans"] == 24


# ---- timed passes ----

@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("bits", BITS)
def test_timed_kernels_make_one_kernel_per_query(setup, bits, mode):
    eng, _, queries, want = setup
    on_mirror(eng, bits, share=1)
    timed0 = eng.stats().scan_kernels_timed
    eng.setTuning("time_kernels", mode)
    try:
        got, d = pipelined(eng, queries[:13], KS[bits][:13], 4, sync=False)
    finally:
        eng.setTuning("time_kernels", 0)
    assert same(got, want[bits][:13])
    assert d["mirror_shared_passes"] == 0 and d["mirror_passes"] == 13 and d["mirror_scans"] == 13 and d["done_flag_waits"] == 0
    assert eng.stats().scan_kernels_timed - timed0 == 13
