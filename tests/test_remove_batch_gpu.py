"""removeBatch (wax_hip_remove_batch): after the call the engine must be in exactly the state a FRESH engine has that addBatch'ed the
surviving rows in order (and, at small sizes, an engine that ran the existing remove loop): equal count, byte-identical serialize(),
and array_equal ids and scores from search, searchBatch (256 queries), searchFiltered and searchBatchFiltered. No test asserts a
time."""
import threading

import numpy as np
import pytest

import oracle
from helpers import OracleEngine, assert_parity

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def wax(hip_lib):
    import wax_amd
    if hip_lib.wax_hip_device_count() == 0:
        pytest.skip("no HIP device on this host: the gpu-marked tests run on the MI355X box (pytest -m gpu)")
    assert hip_lib.wax_hip_available() == 1, "a HIP device is visible but it is not gfx950: the HIP path needs an MI355X"
    return wax_amd


def corpus_for(metric, n, dims, seed=0):
    x = oracle.gaussian_unit_rows(seed, n, dims)
    if metric != 0:   # dot / l2: rows of different norms
        x = x * np.random.default_rng(seed + 7).uniform(0.5, 2.0, size=(n, 1)).astype(np.float32)
    return np.ascontiguousarray(x, dtype=np.float32)


def frame_ids(n):
    """Frame ids that are not row numbers (3 r + 7): an id / row mix-up cannot pass."""
    return np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(7)


def make_engine(wax, metric, dims, corpus=None, ids=None, **kw):
    eng = wax.HIPVectorEngine(metric=wax.VectorMetric(metric), dimensions=dims, **kw)
    if corpus is not None and len(corpus):
        eng.addBatch(ids, corpus)
    return eng


def noisy_list(rng, ids, present):
    """The frame ids of rows `present`, shuffled, with ~5 % absent ids mixed in and as many present ones repeated."""
    present = np.asarray(present, dtype=np.int64)
    lst = ids[present]
    extra = max(1, len(present) // 20) if len(present) else 0
    if extra:
        absent = rng.integers(3 * len(ids) + 100, 6 * len(ids) + 10 ** 6, size=extra).astype(np.uint64)
        absent = absent - absent % np.uint64(3)            # never of the form 3 r + 7
        lst = np.concatenate([lst, absent, lst[rng.integers(0, len(lst), size=extra)]])
    return rng.permutation(lst)


def assert_same_state(eng, ref, queries, ids_left, ctx, ks=(10,), nfilt=16):
    """`eng` against the yardstick engine `ref`: count, serialize bytes, and the four search entry points."""
    assert eng.count == ref.count, f"{ctx}: count {eng.count} != {ref.count}"
    assert eng.serialize() == ref.serialize(), f"{ctx}: serialize() differs"
    if ref.count == 0:
        assert eng.search(queries[0], 10) == [], f"{ctx}: an empty engine returns nothing"
        return
    rng = np.random.default_rng(len(ids_left))
    for k in ks:
        for q in queries[:4]:
            a, b = eng.searchArrays(q, k), ref.searchArrays(q, k)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), f"{ctx}: search k={k}"
        a, b = eng.searchBatch(queries, k), ref.searchBatch(queries, k)
        for x, y, what in zip(a, b, ("ids", "scores", "counts")):
            assert np.array_equal(x, y), f"{ctx}: searchBatch k={k} {what}"
        # allow-lists over survivors and strangers (removed / never present ids are ignored by both engines)
        lists = []
        for i in range(nfilt):
            m = min(len(ids_left), (1, 50, 5000)[i % 3])
            lst = rng.choice(ids_left, size=m, replace=False)
            lists.append(np.concatenate([lst, lst[:3] + np.uint64(1)]))
        a, b = eng.searchFiltered(queries[0], k, frameIds=lists[1]), ref.searchFiltered(queries[0], k, frameIds=lists[1])
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), f"{ctx}: searchFiltered k={k}"
        a, b = eng.searchFiltered(queries[1], k, minScore=0.0), ref.searchFiltered(queries[1], k, minScore=0.0)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), f"{ctx}: searchFiltered (minScore) k={k}"
        a = eng.searchBatchFiltered(queries[:nfilt], k, frameIds=lists)
        b = ref.searchBatchFiltered(queries[:nfilt], k, frameIds=lists)
        for x, y, what in zip(a, b, ("ids", "scores", "counts")):
            assert np.array_equal(x, y), f"{ctx}: searchBatchFiltered k={k} {what}"


def fresh_of(wax, metric, dims, corpus, ids, keep):
    return make_engine(wax, metric, dims, corpus[keep], ids[keep])


# ---- 1. metrics x dims x list sizes ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", [384, 768, 100])
@pytest.mark.parametrize("metric", [0, 1, 2], ids=["cosine", "dot", "l2"])
def test_lists_of_every_size(wax, metric, dims):
    n = 20_000
    corpus, ids = corpus_for(metric, n, dims), frame_ids(n)
    queries = oracle.gaussian_unit_queries(256, dims)
    rng = np.random.default_rng(100 * metric + dims)
    for size in (1, 7, 1000, 19_999, n):
        present = rng.permutation(n)[:size]
        lst = noisy_list(rng, ids, present)
        eng = make_engine(wax, metric, dims, corpus, ids)
        removed = eng.removeBatch(lst)
        assert removed == size, f"out_removed {removed} != distinct present ids {size}"
        keep = np.ones(n, dtype=bool)
        keep[present] = False
        ref = fresh_of(wax, metric, dims, corpus, ids, keep)
        assert_same_state(eng, ref, queries, ids[keep], f"metric {metric} dims {dims} list {size}")
        eng.close()
        ref.close()


def test_equals_the_remove_loop_and_the_oracle(wax):
    """Small size: the same list through the existing remove loop, and one parity check against the CPU oracle."""
    n, dims = 3000, 384
    corpus, ids = corpus_for(0, n, dims, seed=3), frame_ids(n)
    rng = np.random.default_rng(9)
    present = rng.permutation(n)[:400]
    lst = noisy_list(rng, ids, present)
    eng = make_engine(wax, 0, dims, corpus, ids)
    loop = make_engine(wax, 0, dims, corpus, ids)
    assert eng.removeBatch(lst) == 400
    for fid in lst:
        loop.remove(int(fid))
    queries = oracle.gaussian_unit_queries(256, dims)
    keep = np.ones(n, dtype=bool)
    keep[present] = False
    assert_same_state(eng, loop, queries, ids[keep], "removeBatch against the remove loop")
    ref = OracleEngine(0, dims)
    ref.ids, ref.rows = [int(i) for i in ids[keep]], list(corpus[keep])
    for q in queries[:3]:
        got, exp = eng.search(q, 10), ref.search(q, 10)
        assert_parity([h[0] for h in got], [h[1] for h in got], [h[0] for h in exp], [h[1] for h in exp], ctx="oracle parity")
    assert eng.serialize() == ref.serialize()
    eng.close()
    loop.close()


# ---- 2. patterns x window sizes ----------------------------------------------------------------------------------------------------

N2, D2 = 20_000, 384
PATTERNS = {
    "empty": lambda n: np.zeros(0, dtype=np.int64),
    "only_absent": lambda n: None,
    "first_row": lambda n: np.array([0]),
    "last_row": lambda n: np.array([n - 1]),
    "front_block": lambda n: np.arange(0, 3000),
    "middle_block": lambda n: np.arange(7000, 10_000),       # starts and ends on multiples of 1 000: run boundaries on window boundaries
    "end_block": lambda n: np.arange(n - 3000, n),
    "every_second": lambda n: np.arange(0, n, 2),
    "all_but_one": lambda n: np.delete(np.arange(n), 12_345),
    "everything": lambda n: np.arange(n),
    "runs_on_window_edges": lambda n: np.concatenate([np.arange(37, 74), np.arange(999, 2001), np.arange(5000, 5037), [n - 37]]),
}


@pytest.fixture(scope="module")
def small(wax):
    corpus, ids = corpus_for(0, N2, D2, seed=1), frame_ids(N2)
    return corpus, ids, oracle.gaussian_unit_queries(256, D2)


@pytest.mark.parametrize("window", [0, 1000, 37])
@pytest.mark.parametrize("pattern", sorted(PATTERNS))
def test_patterns_and_windows(wax, small, pattern, window):
    corpus, ids, queries = small
    rows = PATTERNS[pattern](N2)
    eng = make_engine(wax, 0, D2, corpus, ids)
    eng.setTuning("compact_window_rows", window)
    assert eng.getTuning("compact_window_rows") == window
    if rows is None:
        lst = np.array([1, 2, 3 * N2 + 1000, 2 ** 63 + 11], dtype=np.uint64)      # none of the form 3 r + 7 below 3 n + 7
        rows = np.zeros(0, dtype=np.int64)
    else:
        lst = np.random.default_rng(5).permutation(ids[rows])
    removed = eng.removeBatch(lst)
    assert removed == len(rows)
    keep = np.ones(N2, dtype=bool)
    keep[rows] = False
    ref = fresh_of(wax, 0, D2, corpus, ids, keep)
    assert_same_state(eng, ref, queries, ids[keep], f"pattern {pattern} window {window}")
    if pattern == "everything":
        assert eng.count == 0 and eng.search(queries[0], 10) == []
        eng.addBatch(ids[:10], corpus[:10])                   # and the emptied engine still takes rows
        assert [h[0] for h in eng.search(corpus[3], 1)] == [int(ids[3])]
    eng.close()
    ref.close()


# ---- 3. rows still staged on the host ----------------------------------------------------------------------------------------------

def test_staged_single_adds_are_among_the_ids(wax):
    n, dims, extra = 5000, 384, 50
    corpus, ids = corpus_for(0, n + extra, dims, seed=2), frame_ids(n + extra)
    eng = make_engine(wax, 0, dims, corpus[:n], ids[:n])
    for r in range(n, n + extra):
        eng.add(int(ids[r]), corpus[r])                      # staged: no reader has flushed them
    rng = np.random.default_rng(4)
    rows = np.concatenate([rng.choice(n, 100, replace=False), n + rng.choice(extra, 20, replace=False)])
    assert eng.removeBatch(rng.permutation(ids[rows])) == 120
    keep = np.ones(n + extra, dtype=bool)
    keep[rows] = False
    ref = fresh_of(wax, 0, dims, corpus, ids, keep)
    assert_same_state(eng, ref, oracle.gaussian_unit_queries(256, dims), ids[keep], "staged adds")
    eng.close()
    ref.close()


# ---- 4. the mirror stays in step ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("single", [False, True], ids=["searchBatch", "scan_mirror_2"])
def test_mirror_is_compacted_not_converted_again(wax, single):
    n, dims = 20_000, 384
    corpus, ids = corpus_for(0, n, dims, seed=6).copy(), frame_ids(n)
    queries = oracle.gaussian_unit_queries(256, dims)
    eng = make_engine(wax, 0, dims, corpus, ids)
    if single:
        eng.setTuning("scan_mirror", 2)
        eng.searchArrays(queries[0], 10)
    else:
        eng.searchBatch(queries, 10)                          # mirror built
    assert eng.getTuning("mirror_rows_converted") >= n
    rng = np.random.default_rng(8)
    dirty = rng.choice(n, 6, replace=False)
    fresh_rows = corpus_for(0, 6, dims, seed=77)
    for r, v in zip(dirty, fresh_rows):                       # upserts: listed as dirty rows of the mirror
        eng.add(int(ids[r]), v)
        corpus[r] = v
    rows = np.concatenate([rng.choice(n, 500, replace=False), dirty[:2]])
    rows = np.unique(rows)
    before = eng.getTuning("mirror_rows_converted")
    assert eng.removeBatch(rng.permutation(ids[rows])) == len(rows)
    keep = np.ones(n, dtype=bool)
    keep[rows] = False
    ref = fresh_of(wax, 0, dims, corpus, ids, keep)
    if single:
        for q in queries[:8]:
            a, b = eng.searchArrays(q, 10), ref.searchArrays(q, 10)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    else:
        a, b = eng.searchBatch(queries, 10), ref.searchBatch(queries, 10)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
    grown = eng.getTuning("mirror_rows_converted") - before
    print(f"mirror rows converted after removeBatch: {grown} (dirty rows: {len(dirty)})")
    assert grown <= len(dirty), f"{grown} mirror rows were converted again; only the {len(dirty)} upserted ones may be"
    assert_same_state(eng, ref, queries, ids[keep], "mirror in step")
    eng.close()
    ref.close()


# ---- 5. one pass, by the bytes written ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mirror", [False, True], ids=["store_only", "with_mirror"])
def test_one_pass_by_bytes_written(wax, small, mirror):
    corpus, ids, queries = small
    bpr = D2 * 4 + 8 + ((D2 * 2 + 4) if mirror else 0)
    window = 1000

    def engine():
        e = make_engine(wax, 0, D2, corpus, ids)
        e.setTuning("compact_window_rows", window)
        if mirror:
            e.searchBatch(queries, 10)
        return e

    # scattered ids: every surviving row behind the first removed one is written at most twice (bounce, then its place)
    eng = engine()
    rows = np.random.default_rng(12).choice(N2, 50, replace=False)
    b0, c0 = eng.getTuning("remove_batch_bytes_written"), eng.getTuning("remove_batches")
    assert eng.removeBatch(ids[rows]) == 50
    written = eng.getTuning("remove_batch_bytes_written") - b0
    behind = N2 - int(rows.min())
    print(f"scattered: {written} bytes written, bound {2 * behind * bpr}")
    assert 0 < written <= 2 * behind * bpr
    assert eng.getTuning("remove_batches") == c0 + 1 and eng.getTuning("remove_batch_rows") >= 50
    eng.close()
    # a list whose first window already shifts by more than its length: every row moves directly, once
    eng = engine()
    rows = np.arange(100, 100 + 2 * window + 100)
    b0 = eng.getTuning("remove_batch_bytes_written")
    assert eng.removeBatch(ids[rows]) == len(rows)
    written = eng.getTuning("remove_batch_bytes_written") - b0
    behind = N2 - 100
    print(f"direct: {written} bytes written, bound {behind * bpr + window * bpr}")
    assert 0 < written <= behind * bpr + window * bpr
    keep = np.ones(N2, dtype=bool)
    keep[rows] = False
    ref = fresh_of(wax, 0, D2, corpus, ids, keep)
    assert_same_state(eng, ref, queries, ids[keep], "direct form")
    eng.close()
    ref.close()


# ---- 6. full size ------------------------------------------------------------------------------------------------------------------

def test_one_million_rows(wax):
    n, dims = 1_000_000, 384
    corpus, ids = corpus_for(0, n, dims), frame_ids(n)
    queries = oracle.gaussian_unit_queries(256, dims)
    rng = np.random.default_rng(21)
    eng = make_engine(wax, 0, dims, corpus, ids)
    eng.searchBatch(queries, 10)                              # the mirror is there, as on a serving engine
    keep = np.ones(n, dtype=bool)
    order = rng.permutation(n)
    for step, rows in enumerate((order[:10_000], order[10_000:11_000])):
        lst = noisy_list(rng, ids, rows)
        assert eng.removeBatch(lst) == len(rows)
        keep[rows] = False
        ref = fresh_of(wax, 0, dims, corpus, ids, keep)
        assert_same_state(eng, ref, queries, ids[keep], f"1M rows, step {step}", ks=(10, 300), nfilt=8)
        ref.close()
    eng.close()


# ---- 7. locking --------------------------------------------------------------------------------------------------------------------

def test_refused_while_the_thread_holds_a_ticket(wax, small):
    corpus, ids, queries = small
    eng = make_engine(wax, 0, D2, corpus[:2000], ids[:2000])
    t = eng.submit(queries[0], 10)
    from wax_amd.errors import EncodingError
    with pytest.raises(EncodingError, match="collect outstanding search tickets first"):
        eng.removeBatch(ids[:5])
    eng.collect(t, 10)
    assert eng.count == 2000
    assert eng.removeBatch(ids[:5]) == 5
    eng.close()


def test_searches_in_other_threads(wax, small):
    corpus, ids, queries = small
    n = 20_000
    eng = make_engine(wax, 0, D2, corpus, ids)
    rows = np.random.default_rng(31).choice(n, 4000, replace=False)
    gone = set(int(i) for i in ids[rows])
    returned = threading.Event()
    stop = threading.Event()
    errors = []

    def reader(seed):
        r = np.random.default_rng(seed)
        try:
            while not stop.is_set():
                after = returned.is_set()
                q = corpus[int(r.integers(0, n))]
                if seed % 2:
                    got = [int(i) for i in eng.searchArrays(q, 10)[0]]
                else:
                    got = [int(i) for i in eng.searchBatch(queries[:16], 10)[0].reshape(-1)]
                assert got, "a search during removeBatch returned nothing"
                if after:
                    assert not gone.intersection(got), "a search that started after removeBatch returned names a removed id"
        except BaseException as exc:   # noqa: BLE001 — reported by the main thread
            errors.append(exc)

    threads = [threading.Thread(target=reader, args=(s,)) for s in range(4)]
    for t in threads:
        t.start()
    try:
        assert eng.removeBatch(ids[rows]) == 4000
        returned.set()
        for _ in range(20):
            eng.searchArrays(queries[0], 10)
    finally:
        stop.set()
        for t in threads:
            t.join()
    assert not errors, errors[0]
    keep = np.ones(n, dtype=bool)
    keep[rows] = False
    ref = fresh_of(wax, 0, D2, corpus, ids, keep)
    assert_same_state(eng, ref, queries, ids[keep], "after concurrent searches")
    eng.close()
    ref.close()


# ---- 8. sharded handle -------------------------------------------------------------------------------------------------------------

def test_sharded_handle_equals_single_engine(wax):
    n, dims = 3072, 384                                       # three blocks of 1 024 rows
    corpus, ids = corpus_for(0, n, dims, seed=4), frame_ids(n)
    queries = oracle.gaussian_unit_queries(256, dims)
    sh = wax.HIPVectorEngine(metric=wax.VectorMetric(0), dimensions=dims, devices=[0, 0, 0])
    sh.setTuning("shard_min_mb", 0)
    one = make_engine(wax, 0, dims)
    for e in (sh, one):
        e.addBatch(ids, corpus)
    info = [sh.shardInfo(g) for g in range(sh.shardCount)]
    assert [i[2] for i in info] == [1024, 1024, 1024], info
    rng = np.random.default_rng(41)
    rows = np.concatenate([rng.choice(1024, 100, replace=False), np.arange(1024, 2048), 2048 + rng.choice(1024, 300, replace=False)])
    lst = noisy_list(rng, ids, rows)
    assert sh.removeBatch(lst) == len(rows)
    assert one.removeBatch(lst) == len(rows)
    info = [sh.shardInfo(g) for g in range(sh.shardCount)]
    assert [i[2] for i in info] == [924, 0, 724], info
    base = 0
    for _, b, r in info:
        assert b == base, f"shard bases are not contiguous: {info}"
        base += r
    keep = np.ones(n, dtype=bool)
    keep[rows] = False
    assert_same_state(sh, one, queries, ids[keep], "sharded handle")
    ref = fresh_of(wax, 0, dims, corpus, ids, keep)
    assert_same_state(one, ref, queries, ids[keep], "single engine against a fresh one")
    for e in (sh, one, ref):
        e.close()
