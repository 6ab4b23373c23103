"""GPU parity tests (run with -m gpu on an MI355X): HIPVectorEngine — i.e. libwaxhip's HIP
kernels through the C ABI — against the CPU oracle on the same seeded inputs, the committed
golden fixtures, the reference's own test cases, and size-independent properties at the
BASELINE.json sizes. Tolerances: scores within 1e-5 (north_star); ids identical except inside
near-tie groups (< 2e-5 apart in the oracle), see helpers.assert_parity."""
import hashlib
import threading

import numpy as np
import pytest

import oracle
from helpers import OracleEngine, assert_parity, load_golden, run_reference_case

pytestmark = pytest.mark.gpu

REF = load_golden("reference_cases.json")
VEC = load_golden("oracle_vectors.json")
MARGIN = 8


@pytest.fixture(scope="module")
def wax(hip_lib):
    import wax_amd
    if hip_lib.wax_hip_device_count() == 0:
        pytest.skip("no HIP device on this host: the gpu-marked tests run on the MI355X box (pytest -m gpu)")
    assert hip_lib.wax_hip_available() == 1, "a HIP device is visible but it is not gfx950: the HIP path needs an MI355X"
    return wax_amd


def make_engine(wax, metric, dims, corpus=None, ids=None):
    eng = wax.HIPVectorEngine(metric=wax.VectorMetric(metric), dimensions=dims)
    if corpus is not None and len(corpus):
        eng.addBatch(np.arange(len(corpus), dtype=np.uint64) if ids is None else ids, corpus)
    return eng


def check(eng, metric, corpus, ids, q, k, ctx):
    got_ids, got_scores = eng.searchArrays(q, k)
    e_ids, e_scores, _, _ = oracle.search(metric, corpus, ids, q, k)
    x_ids, x_scores, _, _ = oracle.search(metric, corpus, ids, q, min(oracle.clamp_topk(k) + MARGIN, 10000))
    assert_parity(got_ids, got_scores, e_ids, e_scores, x_scores, ctx)
    return got_ids, got_scores


# ---------------------------------------------------------------------------
# the reference's own tests, replayed on the HIP engine

@pytest.mark.parametrize("case", REF["engine_cases"], ids=lambda c: c["name"])
def test_reference_cases(wax, case):
    run_reference_case(case, lambda m, d: wax.HIPVectorEngine(metric=wax.VectorMetric(m), dimensions=d),
                       wax.VectorMath.normalizeL2)


def test_reference_dimension_mismatch_and_empty(wax):
    c = REF["dimension_mismatch"]
    eng = wax.HIPVectorEngine(dimensions=c["dimensions"])
    assert eng.search([1.0] * c["query_len"], 5) == []  # empty engine returns [] before validating (:448-449)
    eng.add(0, [1.0] * c["dimensions"])
    with pytest.raises(wax.EncodingError) as ei:
        eng.search([1.0] * c["query_len"], 5)
    assert str(ei.value) == c["message"]
    with pytest.raises(wax.EncodingError) as ei:
        eng.add(1, [1.0] * c["query_len"])
    assert str(ei.value) == c["message"]
    with pytest.raises(wax.EncodingError):
        eng.addBatch([1, 2], [[1.0] * c["dimensions"]])
    assert len(eng.search([1.0] * c["dimensions"], 0)) == 1      # topK < 1 => 1 (:843)
    assert len(eng.search([1.0] * c["dimensions"], -7)) == 1
    assert len(eng.search([1.0] * c["dimensions"], 10 ** 6)) == 1  # clamp to 10000, then min(count)


def test_minilm_fixture_eight_way_tie(wax):
    fx = REF["minilm_fixture"]
    rows = np.full((fx["count"], fx["dimensions"]), 1.0, dtype=np.float32)
    eng = make_engine(wax, 0, fx["dimensions"], rows, np.arange(100, 108, dtype=np.uint64))
    ids, scores = eng.searchArrays(rows[3], 5)
    assert list(ids) == [100, 101, 102, 103, 104]
    assert np.allclose(scores, 1.0, atol=1e-6)


# ---------------------------------------------------------------------------
# committed golden vectors (oracle outputs frozen in tests/golden/oracle_vectors.json)

def _golden_inputs(case):
    n, d = case["n"], case["d"]
    if case["generator"] == "gauss":
        return oracle.gaussian_unit_rows(0, n, d), oracle.gaussian_unit_queries(3, d)
    if case["generator"] == "lcg":
        return (np.stack([oracle.deterministic_embed(f"doc-{i}", d) for i in range(n)]),
                np.stack([oracle.deterministic_embed(f"query-{i}", d) for i in range(3)]))
    return oracle.tie_pattern(0, n, d), np.abs(oracle.gaussian_unit_queries(3, d))


@pytest.mark.parametrize("case", VEC["cases"], ids=lambda c: c["name"])
def test_golden_vectors(wax, case):
    corpus, queries = _golden_inputs(case)
    assert hashlib.sha256(corpus.astype("<f4").tobytes()).hexdigest() == case["corpus_sha256"]
    eng = make_engine(wax, case["metric"], case["d"], corpus)
    for qi, exp in enumerate(case["results"]):
        got_ids, got_scores = eng.searchArrays(queries[qi], case["k"])
        _, x_scores, _, _ = oracle.search(case["metric"], corpus, None, queries[qi], case["k"] + MARGIN)
        assert_parity(got_ids, got_scores, exp["ids"], exp["scores"], x_scores, f"{case['name']} q{qi}")


# ---------------------------------------------------------------------------
# seeded sweeps against the live oracle

SPECIALISED = [64, 128, 256, 384, 512, 768, 1024, 1536]
GENERIC = [1, 2, 3, 4, 6, 20, 100, 388, 2048]


@pytest.mark.parametrize("metric", [0, 1, 2])
@pytest.mark.parametrize("dims", SPECIALISED + GENERIC)
def test_dims_and_metrics(wax, dims, metric):
    n = 2500
    corpus = oracle.gaussian_unit_rows(0, n, dims)
    if metric != 0:
        corpus = corpus * np.linspace(0.5, 2.0, n, dtype=np.float32)[:, None]  # non-unit rows
    ids = (np.arange(n, dtype=np.uint64) * 7 + 3)
    eng = make_engine(wax, metric, dims, corpus, ids)
    for qi, q in enumerate(oracle.gaussian_unit_queries(2, dims)):
        for k in (1, 10, 30):
            check(eng, metric, corpus, ids, q, k, f"d{dims} m{metric} q{qi} k{k}")


@pytest.mark.parametrize("k", [1, 2, 10, 30, 63, 64, 65, 128, 191, 192, 193, 256, 1000, 4999, 5000, 10000, 20000])
def test_k_sweep_fused_and_general_paths(wax, k):
    n, dims = 5000, 128
    corpus = oracle.gaussian_unit_rows(0, n, dims)
    eng = make_engine(wax, 0, dims, corpus)
    q = oracle.gaussian_unit_queries(1, dims)[0]
    ids, scores = check(eng, 0, corpus, None, q, k, f"k{k}")
    assert len(ids) == min(oracle.clamp_topk(k), n)
    assert np.all(np.diff(scores) <= 0)


@pytest.mark.parametrize("n", [1, 2, 3, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 255, 256, 257, 999, 1000, 1001, 8191, 8193])
def test_ragged_row_counts(wax, n):
    for dims in (384, 768, 100):
        corpus = oracle.gaussian_unit_rows(0, n, dims)
        eng = make_engine(wax, 0, dims, corpus)
        q = oracle.gaussian_unit_queries(1, dims)[0]
        check(eng, 0, corpus, None, q, 10, f"n{n} d{dims}")
        check(eng, 0, corpus, None, corpus[n - 1], 1, f"n{n} d{dims} last-row")  # the tail row is reachable


@pytest.mark.parametrize("n,dims,metric", [(300_000, 384, 0), (60_000, 128, 2), (150_000, 768, 1), (80_000, 100, 0), (1_100_000, 128, 0)])
def test_short_selection_equals_the_long_path(wax, n, dims, metric):
    """top_k > 192 ("select_short", default 1): the fused scan leaves every workgroup's 192 best, one workgroup selects the top_k among
    them and certifies that nothing was dropped; the distance pass + radix selection behind it only runs when that fails. Same hits,
    bit for bit, as the long path alone ("select_short" 0) and as the oracle, for every k up to the clamp; no certificate fails on an
    iid corpus."""
    corpus = oracle.gaussian_unit_rows(3, n, dims)
    if metric != 0:
        corpus = corpus * np.linspace(0.5, 2.0, n, dtype=np.float32)[:, None]
    eng = make_engine(wax, metric, dims, corpus)
    assert eng.getTuning("select_short") == 1
    q = oracle.gaussian_unit_queries(2, dims, seed=9)
    grid = eng.getTuning("scan_grid")
    tried = 0
    for k in (193, 300, 1000, 4096, 4097, 7000, 10000):
        # (tried while the lists can hold the answer — k <= 64 per list on average —, their first 2k / lists entries fit the LDS buffer,
        # and the store has at least 256 rows per wanted key)
        ke = min(k, n)
        per_list = 64 if ke <= grid * 8 else 192
        viable = grid * min(per_list, max(4, -(-2 * ke // grid))) <= 16384 and 3 * ke <= grid * per_list and n >= 256 * ke
        tried += viable
        eng.setTuning("select_short", 1)
        before, fails = eng.getTuning("short_selects"), eng.getTuning("short_select_failures")
        a = [eng.searchArrays(qi, k) for qi in q]
        assert eng.getTuning("short_selects") - before == (len(q) if viable else 0), (k, grid)
        assert eng.getTuning("short_select_failures") == fails, k
        eng.setTuning("select_short", 0)
        b = [eng.searchArrays(qi, k) for qi in q]
        assert eng.getTuning("short_selects") - before == (len(q) if viable else 0)
        for (ia, sa), (ib, sb) in zip(a, b):
            assert len(ia) == min(k, n) and np.array_equal(ia, ib) and np.array_equal(sa, sb), k
    assert tried >= (4 if n >= 1_048_576 else 3 if n >= 256_000 else 1), (grid, tried)
    eng.setTuning("select_short", 1)
    check(eng, metric, corpus, None, q[0], 300, "short selection against the oracle")
    eng.setTuning("select_short", 2)                       # 192-entry lists whatever k: the same hits again
    for k in (193, 1000):
        ia, sa = eng.searchArrays(q[0], k)
        eng.setTuning("select_short", 1)
        ib, sb = eng.searchArrays(q[0], k)
        eng.setTuning("select_short", 2)
        assert np.array_equal(ia, ib) and np.array_equal(sa, sb)
    with pytest.raises(Exception):
        eng.setTuning("select_short", 3)
    eng.close()


@pytest.mark.parametrize("layout", ["iid", "sorted"])
def test_short_merge_of_the_fused_path_equals_the_wave_list_merge(wax, layout):
    """64 < top_k <= 192 on a store whose scan does not merge in its own kernel: the per-workgroup lists are merged by the short
    selection ("select_short" 1) — same hits as the wave-list merge ("select_short" 0), on an iid corpus and on one whose best rows
    are its first rows (only a few workgroups' lists hold the answer)."""
    n, dims = 300_000, 384
    corpus = oracle.gaussian_unit_rows(21, n, dims)
    q = oracle.gaussian_unit_queries(2, dims, seed=4)
    if layout == "sorted":
        order = np.argsort(-(corpus @ q[0]), kind="stable")
        corpus = np.ascontiguousarray(corpus[order])
    eng = make_engine(wax, 0, dims, corpus)
    for k in (64, 65, 100, 150, 192):
        eng.setTuning("select_short", 1)
        before, f0 = eng.getTuning("short_selects"), eng.getTuning("short_select_failures")
        a = [eng.searchArrays(qi, k) for qi in q]
        assert eng.getTuning("short_selects") - before == (len(q) if k > 64 else 0), k
        assert eng.getTuning("short_select_failures") == f0
        eng.setTuning("select_short", 0)
        b = [eng.searchArrays(qi, k) for qi in q]
        for (ia, sa), (ib, sb) in zip(a, b):
            assert len(ia) == k and np.array_equal(ia, ib) and np.array_equal(sa, sb), k
    eng.setTuning("select_short", 1)
    check(eng, 0, corpus, None, q[0], 192, f"short merge, {layout}")
    eng.close()


def test_short_selection_certificate_fails_when_one_workgroup_holds_the_answer(wax):
    """The scan deals 8-row chunks to its waves round-robin; put ~400 near-copies of the query exactly on workgroup 0's chunks. Its list
    keeps 192 of them, the other 200 best rows of the store are gone from the candidates: the certificate must see that (workgroup 0's
    last entry is better than the k-th candidate) and the long path must answer — exactly, every time for k = 193 .. 400; a query far
    from the planted rows certifies."""
    n, dims = 200_000, 384
    corpus = oracle.gaussian_unit_rows(11, n, dims)
    probe = make_engine(wax, 0, dims, corpus[:n])
    grid = probe.getTuning("scan_grid")
    probe.close()
    nwaves = grid * 4
    target = oracle.gaussian_unit_queries(1, dims, seed=77)[0].astype(np.float32)
    rows = np.arange(n)
    mine = ((rows // 8) % nwaves) < 4                  # the rows workgroup 0 reads
    planted = rows[mine]
    assert 250 < len(planted) < 2000, (grid, len(planted))
    rng = np.random.default_rng(5)
    noise = rng.standard_normal((len(planted), dims)).astype(np.float32) * np.linspace(0.01, 0.2, len(planted), dtype=np.float32)[:, None]
    near = target[None, :] + noise / np.sqrt(dims)
    corpus[planted] = near / np.linalg.norm(near, axis=1, keepdims=True)
    eng = make_engine(wax, 0, dims, corpus)
    assert eng.getTuning("scan_grid") == grid
    for k in (193, 250, min(400, len(planted))):
        f0 = eng.getTuning("short_select_failures")
        ids, scores = eng.searchArrays(target, k)
        assert eng.getTuning("short_select_failures") == f0 + 1, k
        assert set(ids.tolist()) <= set(planted.tolist()) and len(ids) == k
        eng.setTuning("select_short", 0)
        ids0, scores0 = eng.searchArrays(target, k)
        eng.setTuning("select_short", 1)
        assert np.array_equal(ids, ids0) and np.array_equal(scores, scores0)
    check(eng, 0, corpus, None, target, 300, "planted rows, long path behind a failed certificate")
    f0 = eng.getTuning("short_select_failures")
    far = oracle.gaussian_unit_queries(1, dims, seed=1234)[0]
    check(eng, 0, corpus, None, far, 300, "a query far from the planted rows")
    assert eng.getTuning("short_select_failures") == f0
    eng.close()


def test_force_general_path_equals_fused(wax):
    n, dims = 20000, 384
    corpus = oracle.gaussian_unit_rows(0, n, dims)
    eng = make_engine(wax, 0, dims, corpus)
    for q in oracle.gaussian_unit_queries(3, dims):
        eng.setTuning("force_general", 0)
        a = eng.searchArrays(q, 30)
        eng.setTuning("force_general", 1)
        b = eng.searchArrays(q, 30)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    eng.setTuning("force_general", 0)


def test_scan_variants_are_bit_identical(wax):
    for dims in (384, 768):
        n = 30000
        corpus = oracle.gaussian_unit_rows(0, n, dims)
        eng = make_engine(wax, 0, dims, corpus)
        q = oracle.gaussian_unit_queries(1, dims)[0]
        base = None
        for variant in range(eng.getTuning("variant_count")):
            for grid in (0, 64, 1000):
                eng.setTuning("variant", variant)
                eng.setTuning("grid_blocks", grid)
                got = eng.searchArrays(q, 10)
                if base is None:
                    base = got
                    check(eng, 0, corpus, None, q, 10, f"variant{variant}")
                assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1]), (dims, variant, grid)


def test_exact_ties_resolve_by_ascending_row(wax):
    n, dims = 5000, 128
    corpus = oracle.tie_pattern(0, n, dims)  # rows i and i+256 are identical
    eng = make_engine(wax, 0, dims, corpus)
    q = np.abs(oracle.gaussian_unit_queries(1, dims)[0])
    for k in (24, 100, 300):
        ids, scores = eng.searchArrays(q, k)
        e_ids, e_scores, _, _ = oracle.search(0, corpus, None, q, k)
        assert np.max(np.abs(scores - e_scores)) <= 1e-5
        rows = ids.astype(np.int64)
        for i in range(len(rows) - 1):
            if scores[i] == scores[i + 1] and rows[i] % 256 == rows[i + 1] % 256:
                assert rows[i] < rows[i + 1]
        dup = n // 256  # each distinct row appears ~19-20 times; the best residue comes first, ascending
        first = rows[:min(k, dup)]
        assert np.all(first % 256 == first[0] % 256) and np.all(np.diff(first) == 256)


def test_special_values(wax):
    dims = 384
    corpus = oracle.gaussian_unit_rows(0, 300, dims)
    corpus[5] = 0.0                      # zero row => similarity 0 (CosineDistance.metal:323)
    corpus[7, 3] = np.nan                # NaN row: `sqrt(m) > 1e-6` is false => similarity 0, like the Metal kernel
    corpus[9] *= np.float32(1e-4)        # tiny but > 1e-6 norm: still a valid direction
    eng = make_engine(wax, 0, dims, corpus)
    q = oracle.gaussian_unit_queries(1, dims)[0]
    ids, scores = eng.searchArrays(q, 300)
    assert len(ids) == 300
    assert scores[list(ids).index(5)] == 0.0 and scores[list(ids).index(7)] == 0.0
    e_ids, e_scores, _, _ = oracle.search(0, corpus, None, q, 300)
    x = dict(zip(e_ids.tolist(), e_scores.tolist()))
    assert max(abs(x[int(i)] - float(s)) for i, s in zip(ids, scores)) <= 1e-5
    # dot metric: a NaN row has a NaN distance => dropped on the host (MetalVectorEngine.swift:597)
    deng = make_engine(wax, 1, dims, corpus)
    dids, dscores = deng.searchArrays(q, 300)
    assert 7 not in dids and len(dids) == 299 and np.all(np.isfinite(dscores))
    # +inf component => NaN/inf distance under l2 => dropped as well
    corpus2 = corpus.copy()
    corpus2[7] = corpus[8]
    corpus2[11, 0] = np.inf
    leng = make_engine(wax, 2, dims, corpus2)
    lids, lscores = leng.searchArrays(q, 300)
    assert 11 not in lids and len(lids) == 299
    # zero query: every similarity is 0 => first k rows by index
    zids, zscores = eng.searchArrays(np.zeros(dims, np.float32), 4)
    assert list(zids) == [0, 1, 2, 3] and np.all(zscores == 0.0)
    # scaled query: same ranking, same scores (true cosine)
    a = eng.searchArrays(q, 10)
    b = eng.searchArrays(q * np.float32(12.0), 10)
    assert np.array_equal(a[0], b[0]) and np.max(np.abs(a[1] - b[1])) < 1e-6


# ---------------------------------------------------------------------------
# store semantics (a9) and persistence

def test_random_upsert_remove_sequence_matches_reference_semantics(wax):
    dims = 384
    rng = np.random.default_rng(5)
    eng = wax.HIPVectorEngine(dimensions=dims)
    ref = OracleEngine(0, dims)
    pool = oracle.gaussian_unit_rows(0, 600, dims)
    q = oracle.gaussian_unit_queries(1, dims)[0]
    for step in range(60):
        r = rng.random()
        if r < 0.5:
            m = int(rng.integers(1, 40))
            ids = rng.integers(0, 200, m).tolist()        # collisions with existing ids and inside the batch
            vecs = pool[rng.integers(0, 600, m)]
            eng.addBatch(ids, vecs)
            ref.addBatch(ids, list(vecs))
        elif r < 0.7:
            fid = int(rng.integers(0, 200))
            v = pool[int(rng.integers(0, 600))]
            eng.add(fid, v)
            ref.add(fid, v)
        else:
            fid = int(rng.integers(0, 220))                # sometimes absent => no-op
            eng.remove(fid)
            ref.remove(fid)
        assert eng.count == ref.count
        if ref.count:
            got = eng.searchArrays(q, 10)
            exp = ref.search(q, 10)
            assert_parity(got[0], got[1], [e[0] for e in exp], [e[1] for e in exp], ctx=f"step{step}")
    assert eng.serialize() == ref.serialize()              # same rows in the same order, byte for byte


def test_capacity_growth_preserves_rows(wax):
    dims = 64
    eng = wax.HIPVectorEngine(dimensions=dims)
    corpus = oracle.gaussian_unit_rows(0, 1000, dims)
    assert eng.stats().reserved_rows == REF["constants"]["initial_reserve"]
    for i in range(0, 1000, 37):                           # crosses 64 -> 128 -> ... -> 1024
        eng.addBatch(np.arange(i, min(i + 37, 1000), dtype=np.uint64), corpus[i:i + 37])
    assert eng.stats().reserved_rows == 1024
    assert eng.serialize() == oracle.mv2v_serialize(0, corpus, np.arange(1000, dtype=np.uint64))


@pytest.mark.parametrize("metric", [0, 1, 2])
def test_serialize_is_byte_identical_and_roundtrips(wax, metric):
    dims, n = 384, 777
    corpus = oracle.gaussian_unit_rows(0, n, dims)
    ids = np.arange(n, dtype=np.uint64)[::-1].copy() + 2 ** 40
    eng = make_engine(wax, metric, dims, corpus, ids)
    blob = eng.serialize()
    assert blob == oracle.mv2v_serialize(metric, corpus, ids)
    kind, info, v2, i2 = wax.VectorSerializer.decodeVecSegment(blob)
    assert kind == "metal" and np.array_equal(v2, corpus) and np.array_equal(i2, ids)
    eng2 = wax.HIPVectorEngine(metric=wax.VectorMetric(metric), dimensions=dims)
    eng2.deserialize(blob)
    q = oracle.gaussian_unit_queries(1, dims)[0]
    a, b = eng.searchArrays(q, 20), eng2.searchArrays(q, 20)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    eng2.add(int(ids[5]), corpus[0])                        # id map rebuilt by deserialize: this is an update
    assert eng2.count == n
    assert eng.serialize() == blob                          # serialize does not mutate
    empty = wax.HIPVectorEngine(metric=wax.VectorMetric(metric), dimensions=dims)
    eb = empty.serialize()
    assert eb == oracle.mv2v_serialize(metric, np.zeros((0, dims), np.float32), np.zeros(0, np.uint64)) and len(eb) == 44
    eng2.deserialize(eb)
    assert eng2.count == 0 and eng2.search(q, 5) == []


def test_deserialize_rejects_malformed_segments(wax):
    dims = 8
    corpus = oracle.gaussian_unit_rows(0, 5, dims)
    blob = oracle.mv2v_serialize(0, corpus, np.arange(5, dtype=np.uint64))
    eng = wax.HIPVectorEngine(dimensions=dims)
    cases = {
        "too small": blob[:20],
        "magic mismatch": b"XXXX" + blob[4:],
        "version": blob[:4] + b"\x02\x00" + blob[6:],
        "encoding": blob[:6] + b"\x01" + blob[7:],
        "Metric mismatch": blob[:7] + b"\x01" + blob[8:],
        "Dimension mismatch": blob[:8] + b"\x10\x00\x00\x00" + blob[12:],
        "reserved": blob[:30] + b"\x01" + blob[31:],
        "length mismatch": blob[:20] + b"\x01" + blob[21:],
        "frameId": blob[:-8],
    }
    for reason, bad in cases.items():
        with pytest.raises(wax.InvalidToc) as ei:
            eng.deserialize(bad)
        assert reason.split()[0].lower() in str(ei.value).lower(), (reason, str(ei.value))
    assert eng.count == 0
    eng.deserialize(blob)
    assert eng.count == 5


# ---------------------------------------------------------------------------
# concurrency contract: re-entrant readers, pooled scratch

def test_concurrent_searches_and_pool(wax):
    dims, n = 384, 50000
    corpus = oracle.gaussian_unit_rows(0, n, dims)
    eng = make_engine(wax, 0, dims, corpus)
    queries = oracle.gaussian_unit_queries(16, dims)
    serial = [eng.searchArrays(q, 10) for q in queries]
    results = [None] * len(queries)
    errors = []

    def worker(lo, hi):
        try:
            for _ in range(5):
                for i in range(lo, hi):
                    results[i] = eng.searchArrays(queries[i], 10)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(i * 2, i * 2 + 2)) for i in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for a, b in zip(serial, results):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    st = eng.debugBufferPoolStats()
    assert 1 <= st.transientAllocations <= eng.getTuning("slots") and st.reuseCount > 0
    # pipelined tickets collected out of order
    tickets = [eng.submit(q, 10) for q in queries[:4]]
    for i in (2, 0, 3, 1):
        got = eng.collect(tickets[i], 10)
        assert np.array_equal(got[0], serial[i][0]) and np.array_equal(got[1], serial[i][1])
    # batch API == per-query API
    ids, scores, counts = eng.searchBatch(queries, 10)
    assert np.all(counts == 10)
    for i in range(len(queries)):
        assert np.array_equal(ids[i], serial[i][0]) and np.array_equal(scores[i], serial[i][1])
    # writer while readers are idle: still consistent
    eng.add(10 ** 9, queries[0])
    assert eng.search(queries[0], 1)[0][0] == 10 ** 9


# ---------------------------------------------------------------------------
# sharded path on one GPU: two engines = two shards, merged on device

def test_shard_engines_merge_to_the_single_engine_answer(wax):
    import torch
    dims, n, k = 384, 40000, 10
    corpus = oracle.gaussian_unit_rows(0, n, dims)
    ids = np.arange(n, dtype=np.uint64) + 5000
    whole = make_engine(wax, 0, dims, corpus, ids)
    cuts = [0, 12800, 12800, 30016, n]  # includes an empty shard
    shards = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        e = wax.HIPVectorEngine(dimensions=dims)
        if hi > lo:
            e.addBatchDevice(ids[lo:hi], torch.from_numpy(corpus[lo:hi]).cuda().contiguous())
        e.setRowBase(lo)
        shards.append(e)
    dev = torch.device("cuda", whole.device)
    for q in oracle.gaussian_unit_queries(3, dims):
        parts = [torch.empty((k, 2), dtype=torch.int64, device=dev) for _ in shards]
        st = torch.cuda.current_stream().cuda_stream
        for e, p in zip(shards, parts):
            e.searchShardDevice(q, k, p.data_ptr(), st)
        gathered = torch.cat(parts, dim=0).contiguous()
        merged = torch.empty((k, 2), dtype=torch.int64, device=dev)
        wax.HIPVectorEngine.mergeHitsDevice(gathered.data_ptr(), gathered.shape[0], k, merged.data_ptr(), st)
        torch.cuda.synchronize()
        got = wax.HIPVectorEngine.hitsToResults(wax.VectorMetric.cosine, merged.cpu().numpy())
        exp = whole.searchArrays(q, k)
        assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])  # bit-identical at any shard count
        from wax_amd import sharded
        host = wax.HIPVectorEngine.hitsToResults(wax.VectorMetric.cosine,
                                                 sharded.merge_hits_host(gathered.cpu().numpy(), k))
        assert np.array_equal(host[0], exp[0]) and np.array_equal(host[1], exp[1])
        check(whole, 0, corpus, ids, q, k, "whole")


def test_sharded_searcher_single_rank_pipeline(wax):
    from wax_amd import sharded
    dims, n = 384, 20000
    corpus = oracle.gaussian_unit_rows(0, n, dims)
    eng = make_engine(wax, 0, dims, corpus)
    queries = oracle.gaussian_unit_queries(12, dims)
    for host_merge in (False, True):
        s = sharded.ShardedSearcher(eng, rank=0, world=1, topK=10, depth=4, n_streams=2, host_merge=host_merge)
        out = []
        for i, q in enumerate(queries):
            if len(s.inflight) == s.depth:
                out.append(s.collect())
            s.submit(q)
        while s.inflight:
            out.append(s.collect())
        for q, got in zip(queries, out):
            exp = eng.searchArrays(q, 10)
            assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])


# ---------------------------------------------------------------------------
# BASELINE.json sizes: the HIP answers compared id-for-id with the f64 oracle on the SAME corpus (generated on the
# device, copied to the host once; the oracle's OpenMP f64 scan takes ~20 ms per 1M x 384 rows on the GPU box's host
# cores), plus the size-independent properties (idempotence, shard union, self-retrieval).

def _device_corpus(torch, n, dims, dev, chunk=262144):
    g = torch.Generator(device=dev)
    for lo in range(0, n, chunk):
        g.manual_seed(oracle.CORPUS_SEED + lo // chunk)
        x = torch.randn((min(chunk, n - lo), dims), generator=g, device=dev, dtype=torch.float32)
        yield lo, torch.nn.functional.normalize(x, dim=1).contiguous()


def _load_device_corpus(wax, torch, n, dims, dev, host=True, extra=()):
    """Engine with the n x dims device-generated corpus (frameId = row) and, if asked, its host copy."""
    eng = wax.HIPVectorEngine(dimensions=dims)
    eng.reserve(n)
    corpus = np.empty((n, dims), dtype=np.float32) if host else None
    for lo, x in _device_corpus(torch, n, dims, dev):
        hi = lo + x.shape[0]
        eng.addBatchDevice(np.arange(lo, hi, dtype=np.uint64), x)
        for cb in extra:
            cb(lo, hi, x)
        if host:
            corpus[lo:hi] = x.cpu().numpy()
    assert eng.count == n
    return eng, corpus


def _assert_batch_parity(metric, corpus, queries, k, got_ids, got_scores, got_counts, id_base, ctx):
    """Every query of a batch against oracle.search_batch (one pass over the rows for all queries)."""
    rows, dist, counts = oracle.search_batch(metric, corpus, queries, k + MARGIN)
    for i in range(len(queries)):
        kk = min(k, int(counts[i]))
        e_ids = rows[i, :kk] + id_base
        x_scores = oracle.scores_from_distances(metric, dist[i, :counts[i]])
        assert got_counts[i] == kk, (ctx, i, got_counts[i], kk)
        assert_parity(got_ids[i][:kk], got_scores[i][:kk], e_ids, x_scores[:kk], x_scores, f"{ctx} q{i}")


@pytest.mark.parametrize("metric", [1, 2])
def test_full_size_parity_dot_and_l2(wax, metric):
    """North star: "cosine / dot-product". 1M x 384 with row norms spread over 0.5 .. 2 (l2: 0.5 .. 1; so dot and l2 rank differently
    from cosine): single queries and a 256-query batch (dot: bf16 MFMA one-pass path; l2: LDS-tiled GEMM + slab
    pipeline), every answer id for id against the f64 oracle."""
    import torch
    dev = torch.device("cuda", 0)
    n, dims, k = 1_000_000, 384, 10
    eng = wax.HIPVectorEngine(metric=wax.VectorMetric(metric), dimensions=dims)
    eng.reserve(n)
    corpus = np.empty((n, dims), dtype=np.float32)
    for lo, x in _device_corpus(torch, n, dims, dev):
        hi = lo + x.shape[0]
        spread = 1.5 if metric == 1 else 0.5      # l2 distances grow with the norms: keep them near 1 so that 1e-5 absolute stays meaningful
        scale = 0.5 + spread * ((torch.arange(lo, hi, device=dev, dtype=torch.float32) * 0.6180339887) % 1.0)
        x = (x * scale[:, None]).contiguous()
        eng.addBatchDevice(np.arange(lo, hi, dtype=np.uint64), x)
        corpus[lo:hi] = x.cpu().numpy()
    queries = oracle.gaussian_unit_queries(256, dims, seed=123)
    got = [eng.searchArrays(q, k) for q in queries[:6]]
    _assert_batch_parity(metric, corpus, queries[:6], k, [g[0] for g in got], [g[1] for g in got], [len(g[0]) for g in got], 0,
                         f"metric{metric} single")
    before = eng.getTuning("batch_queries")
    ids, scores, counts = eng.searchBatch(queries, k)
    assert eng.getTuning("batch_queries") - before == 256          # the MFMA path answered
    _assert_batch_parity(metric, corpus, queries, k, list(ids), list(scores), list(counts), 0, f"metric{metric} batch")
    eng.close()


@pytest.mark.parametrize("n,dims,nq", [(1_000_000, 384, 8), (10_000_000, 384, 8), (1_000_000, 768, 3),
                                       (6_000_000, 768, 2)])  # 6M x 768 = 4.6e9 elements: past the reference kernels' 32-bit offset wrap (CosineDistance.metal:191, 275)
def test_full_size_parity_with_oracle(wax, n, dims, nq):
    import torch
    dev = torch.device("cuda", 0)
    half_a, half_b = wax.HIPVectorEngine(dimensions=dims), wax.HIPVectorEngine(dimensions=dims)
    split = (n // 2 // 64) * 64
    do_halves = n <= 1_000_000

    def feed_halves(lo, hi, x):
        if not do_halves:
            return
        if hi <= split:
            half_a.addBatchDevice(np.arange(lo, hi, dtype=np.uint64), x)
        elif lo >= split:
            half_b.addBatchDevice(np.arange(lo, hi, dtype=np.uint64), x)
        else:
            half_a.addBatchDevice(np.arange(lo, split, dtype=np.uint64), x[:split - lo].contiguous())
            half_b.addBatchDevice(np.arange(split, hi, dtype=np.uint64), x[split - lo:].contiguous())

    eng, corpus = _load_device_corpus(wax, torch, n, dims, dev, host=True, extra=(feed_halves,))
    k = 10
    queries = oracle.gaussian_unit_queries(nq, dims)
    got = [eng.searchArrays(q, k) for q in queries]
    # k <= 64: the scan merges in its own kernel (one packet, completion word) up to 2 GiB of rows; beyond, a separate merge kernel
    assert (eng.getTuning("done_flag_waits") == nq) == (n * dims * 4 <= 2 << 30), (n, dims, eng.getTuning("done_flag_waits"))
    # the whole top-10 of every query, id for id and score for score, against the f64 oracle on the same rows
    _assert_batch_parity(0, corpus, queries, k, [g[0] for g in got], [g[1] for g in got], [len(g[0]) for g in got], 0,
                         f"{n}x{dims}")
    for q, (ids, scores) in zip(queries[:3], got[:3]):
        again = eng.searchArrays(q, k)
        assert np.array_equal(ids, again[0]) and np.array_equal(scores, again[1])       # idempotent
        if do_halves:                                                                   # shard-union property
            a = half_a.searchArrays(q, k)
            half_b.setRowBase(split)
            b = half_b.searchArrays(q, k)
            allids = np.concatenate([a[0], b[0]])
            allsc = np.concatenate([a[1], b[1]])
            order = np.lexsort((allids, -allsc.astype(np.float64)))[:k]
            assert np.array_equal(allids[order], ids) and np.array_equal(allsc[order], scores)
    # self-retrieval: a stored row is its own nearest neighbour with score 1
    for r in (0, n // 3, n - 1):
        ids, scores = eng.searchArrays(corpus[r], 1)
        assert ids[0] == r and abs(scores[0] - 1.0) <= 1e-5
    # the timing entry points used by bench.py work at this size
    ms = eng.timeScanKernel(corpus[0], 10, 3)
    rd = eng.timeStreamRead(3)
    assert ms > 0 and rd > 0
    print(f"\n[{n}x{dims}] scan {ms:.3f} ms = {n * dims * 4 / ms / 1e6:.0f} GB/s ; stream-read {rd:.3f} ms = "
          f"{n * dims * 4 / rd / 1e6:.0f} GB/s")
    eng.close(), half_a.close(), half_b.close()


# ---------------------------------------------------------------------------
# batched queries: bf16 MFMA GEMM + select + exact f32 re-score + certificate (BASELINE configs 3 / 5)

@pytest.mark.parametrize("dims,n,nq", [(384, 24 * 256 * 64 + 37, 256), (384, 400_003, 600), (768, 200_011, 700), (128, 24 * 256 * 128 + 5, 200),
                                       (384, 24 * 256 * 64 - 64, 256)])
def test_batch_tail_pool_gives_the_fixed_share_answers(wax, dims, n, nq):
    """The filtering GEMM's workgroups claim the last twelfth of the store's tiles from a pool ("batch_dyn_tail", default 1; one query
    group, stores of at least 24 tiles per workgroup). Which workgroup meets a row must not show: the answers equal those of fixed
    shares ("batch_dyn_tail" 0) and of the single-query path bit for bit — at the smallest store that has a pool (with a ragged last
    tile), with 2 - 4 query groups (fixed shares whatever the key says), and one tile below the threshold (no pool)."""
    corpus = oracle.gaussian_unit_rows(77, n, dims)
    eng = make_engine(wax, 0, dims, corpus)
    assert eng.getTuning("batch_dyn_tail") == 1
    queries = oracle.gaussian_unit_queries(nq, dims, seed=5)
    out = {}
    for dyn in (1, 0, 1):
        eng.setTuning("batch_dyn_tail", dyn)
        before = eng.getTuning("onepass_queries")
        ids, scores, counts = eng.searchBatch(queries, 10)
        assert eng.getTuning("onepass_queries") - before == nq
        if dyn in out:
            assert np.array_equal(ids, out[dyn][0]) and np.array_equal(scores, out[dyn][1])
        out[dyn] = (ids, scores, counts)
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])
    for i in (0, 1, nq // 2, nq - 1):
        s_ids, s_scores = eng.searchArrays(queries[i], 10)
        assert np.array_equal(out[1][0][i], s_ids) and np.array_equal(out[1][1][i], s_scores)
    # the last rows of the store are pool tiles: a query that IS one of them must find it
    probe = corpus[[n - 1, n - 40, n - 3000]].copy()
    ids, scores, counts = eng.searchBatch(np.concatenate([probe, queries[:29]]), 3)
    assert [int(ids[j, 0]) for j in range(3)] == [n - 1, n - 40, n - 3000]
    with pytest.raises(Exception):
        eng.setTuning("batch_dyn_tail", 2)
    eng.close()


def _batch_vs_single(eng, queries, k):
    ids, scores, counts = eng.searchBatch(queries, k)
    for i, q in enumerate(queries):
        s_ids, s_scores = eng.searchArrays(q, k)
        assert counts[i] == len(s_ids), (i, counts[i], len(s_ids))
        assert np.array_equal(ids[i, :counts[i]], s_ids), (i, ids[i, :counts[i]], s_ids)
        assert np.array_equal(scores[i, :counts[i]], s_scores), (i, scores[i, :counts[i]], s_scores)  # bit-identical
    return ids, scores, counts


@pytest.mark.parametrize("metric,dims", [(0, 384), (0, 128), (0, 768), (1, 384), (2, 384), (0, 64), (2, 1024)])
def test_batch_mfma_path_is_exact(wax, metric, dims):
    n, k = 40000, 10
    corpus = oracle.gaussian_unit_rows(0, n, dims)
    if metric != 0:
        corpus = corpus * np.linspace(0.5, 2.0, n, dtype=np.float32)[:, None]
    ids = np.arange(n, dtype=np.uint64) + 77
    eng = make_engine(wax, metric, dims, corpus, ids)
    queries = oracle.gaussian_unit_queries(200, dims)
    before = eng.getTuning("batch_queries")
    b_ids, b_scores, counts = _batch_vs_single(eng, queries, k)
    assert eng.getTuning("batch_queries") - before == 200            # the MFMA path actually ran
    fallbacks = eng.getTuning("batch_fallbacks")
    print(f"\n[batch m{metric} d{dims}] certificate fallbacks: {fallbacks}/200")
    if metric == 0:  # unit-norm cosine: the rank-10 .. rank-64 gap dwarfs the bf16 bound
        assert fallbacks <= 20, f"certificate failed for {fallbacks}/200 random queries"
    for i in (0, 57, 199):                                            # and the answers are the oracle's
        e_ids, e_scores, _, _ = oracle.search(metric, corpus, ids, queries[i], k)
        x = oracle.search(metric, corpus, ids, queries[i], k + MARGIN)[1]
        assert_parity(b_ids[i], b_scores[i], e_ids, e_scores, x, f"batch m{metric} d{dims} q{i}")


def test_batch_edge_shapes(wax):
    dims = 384
    corpus = oracle.gaussian_unit_rows(0, 30000, dims)
    eng = make_engine(wax, 0, dims, corpus)
    for nq, k in [(16, 10), (17, 1), (130, 30), (1029, 10), (64, 80)]:
        _batch_vs_single(eng, oracle.gaussian_unit_queries(nq, dims, seed=100 + nq), k)
    # k above the slab pipeline's limit: the one-pass pipeline takes it since round 6 (30 000 rows >= 64 units of 64 rows) ...
    before = eng.getTuning("batch_queries")
    _batch_vs_single(eng, oracle.gaussian_unit_queries(20, dims), 100)
    assert eng.getTuning("batch_queries") == before + 20
    # ... with the old floor (65 536 rows) it falls back to pipelined single-query scans, and so do batches below batch_min
    eng.setTuning("batch_onepass_tiles", 1024)
    before = eng.getTuning("batch_queries")
    _batch_vs_single(eng, oracle.gaussian_unit_queries(20, dims), 100)
    eng.setTuning("batch_onepass_tiles", 64)
    eng.setTuning("batch_min", 16)
    _batch_vs_single(eng, oracle.gaussian_unit_queries(5, dims), 10)
    assert eng.getTuning("batch_queries") == before
    # default: small batches take the MFMA path when one pass over the bf16 mirror beats nq scans of the f32 store
    eng.setTuning("batch_min", 1)
    _batch_vs_single(eng, oracle.gaussian_unit_queries(8, dims, seed=42), 10)      # 30 000 rows: 8 scans > one GEMM pass
    assert eng.getTuning("batch_queries") == before + 8
    _batch_vs_single(eng, oracle.gaussian_unit_queries(2, dims, seed=43), 10)      # 2 scans are cheaper: loop path
    assert eng.getTuning("batch_queries") == before + 8
    # fewer rows than k': every row is re-scored, certificate is trivially true
    small = make_engine(wax, 0, dims, corpus[:50])
    ids, scores, counts = _batch_vs_single(small, oracle.gaussian_unit_queries(40, dims), 10)
    assert small.getTuning("batch_fallbacks") == 0
    tiny = make_engine(wax, 0, dims, corpus[:3])
    ids, scores, counts = _batch_vs_single(tiny, oracle.gaussian_unit_queries(32, dims), 10)
    assert np.all(counts == 3)
    # tiny score-tile budget => many slabs / segments
    eng.setTuning("batch_slab_mb", 1)
    _batch_vs_single(eng, oracle.gaussian_unit_queries(100, dims, seed=5), 10)
    eng.setTuning("batch_slab_mb", 64)
    # mutation invalidates the bf16 mirror
    probe = oracle.gaussian_unit_queries(32, dims, seed=9)
    eng.add(10 ** 7, probe[3])
    ids, scores, counts = eng.searchBatch(probe, 5)
    assert ids[3, 0] == 10 ** 7 and abs(scores[3, 0] - 1.0) <= 1e-5
    eng.remove(10 ** 7)
    ids, scores, counts = eng.searchBatch(probe, 5)
    assert 10 ** 7 not in ids
    # the loop path gives the same answers
    eng.setTuning("batch_mode", 0)
    l_ids, l_scores, l_counts = eng.searchBatch(probe, 5)
    assert np.array_equal(ids, l_ids) and np.array_equal(scores, l_scores)
    eng.setTuning("batch_mode", 1)


def test_batch_certificate_falls_back_on_ties(wax):
    """Exact duplicates tie in bf16 and in f32: the certificate must refuse them and the exact
    path must still return the (distance asc, row asc) answer."""
    n, dims = 20000, 128
    corpus = oracle.tie_pattern(0, n, dims)
    eng = make_engine(wax, 0, dims, corpus)
    queries = np.abs(oracle.gaussian_unit_queries(48, dims))
    _batch_vs_single(eng, queries, 24)
    assert eng.getTuning("batch_fallbacks") > 0


def test_batch_throughput_config3(wax):
    """BASELINE config 3: 1M x 384, 256 queries, bf16 MFMA + fused select + f32 re-score. EVERY one of the 256
    answers is compared with the f64 oracle (ids + scores), not with the HIP single-query path."""
    import time
    import torch
    n, dims, nq, k = 1_000_000, 384, 256, 10
    dev = torch.device("cuda", 0)
    eng, corpus = _load_device_corpus(wax, torch, n, dims, dev)
    queries = oracle.gaussian_unit_queries(nq, dims)
    eng.searchBatch(queries, k)                       # builds the mirror
    before = eng.getTuning("batch_queries")
    t0 = time.perf_counter()
    reps = 5
    for _ in range(reps):
        ids, scores, counts = eng.searchBatch(queries, k)
    dt = (time.perf_counter() - t0) / reps
    assert eng.getTuning("batch_queries") - before == reps * nq      # the MFMA path served them
    fb = eng.getTuning("batch_fallbacks")
    print(f"\n[config3 1Mx384 Q=256] {dt * 1e3:.2f} ms/batch = {nq / dt:.0f} q/s, "
          f"{2 * nq * n * dims / dt / 1e12:.1f} TFLOP/s bf16, fallbacks so far {fb}")
    t0 = time.perf_counter()
    _assert_batch_parity(0, corpus, queries, k, ids, scores, counts, 0, "config3")
    print(f"[config3] oracle check of all {nq} answers took {time.perf_counter() - t0:.1f} s")
    for i in (0, 100, 255):                           # and bit-identical to the single-query path
        s_ids, s_scores = eng.searchArrays(queries[i], k)
        assert np.array_equal(ids[i], s_ids) and np.array_equal(scores[i], s_scores)
    assert fb <= 3 * 26
    eng.close()


def test_batch_config5_shard_shape(wax):
    """BASELINE config 5, one GPU's share of the 8-way sharded corpus: 1.25M x 768, 1024 queries (K-split
    register-resident GEMM), with row_base set as on rank 3 of 8. ALL 1024 answers are compared with the f64 oracle on the
    same rows (one oracle pass for the whole batch); no certificate fallbacks on random data."""
    import time
    import torch
    n, dims, nq, k = 1_250_000, 768, 1024, 10
    base = 3_750_000
    dev = torch.device("cuda", 0)
    eng, corpus = _load_device_corpus(wax, torch, n, dims, dev)
    eng.setRowBase(base)                              # as rank 3 of 8
    queries = oracle.gaussian_unit_queries(nq, dims, seed=55)
    hits, counts = eng.searchBatchHits(queries, k)    # builds the mirror
    t0 = time.perf_counter()
    reps = 3
    for _ in range(reps):
        hits, counts = eng.searchBatchHits(queries, k)
    dt = (time.perf_counter() - t0) / reps
    fb = eng.getTuning("batch_fallbacks")
    print(f"\n[config5 shard 1.25Mx768 Q=1024] {dt * 1e3:.2f} ms/batch = {nq / dt:.0f} q/s per GPU, "
          f"{2 * nq * n * dims / dt / 1e12:.1f} TFLOP/s bf16, fallbacks so far {fb}")
    assert np.all(counts == k) and np.all((hits[:, :, 0] & 0xFFFFFFFF) >= base)
    from wax_amd import sharded
    h_ids, h_scores, h_valid = sharded.decode_hits(wax.VectorMetric.cosine, hits)
    assert np.all(h_valid)
    sel = np.arange(0, nq)
    # keys carry GLOBAL rows (row_base + local row); frame ids are the local rows here
    assert np.array_equal((hits[:, :, 0] & 0xFFFFFFFF) - base, h_ids.astype(np.int64))
    t0 = time.perf_counter()
    _assert_batch_parity(0, corpus, queries[sel], k, h_ids[sel], h_scores[sel], counts[sel], 0, "config5")
    print(f"[config5] oracle check of {len(sel)} answers took {time.perf_counter() - t0:.1f} s")
    eng.setRowBase(0)
    for i in (0, 511, 1023):
        s_ids, s_scores = eng.searchArrays(queries[i], k)
        assert np.array_equal(h_ids[i], s_ids) and np.array_equal(h_scores[i], s_scores)
    assert fb == 0
    eng.close()


def _oracle_batch_streaming(eng, torch, n, dims, dev, queries, kk, block_rows=1_048_576):
    """Loads the n x dims device-generated corpus into `eng` and returns the f64 oracle's (rows, distances, counts) top-kk
    of every query WITHOUT holding the corpus on the host: rows are downloaded a block at a time, the oracle answers the
    whole batch on the block (oracle.search_batch: one pass for all queries) and the per-query lists are merged by
    (distance asc, row asc) — the oracle's own order. Host memory stays at one block (3 GB at 768 dims) instead of 30 GB."""
    nq = len(queries)
    best_rows = np.full((nq, 0), -1, dtype=np.int64)
    best_dist = np.full((nq, 0), np.inf, dtype=np.float32)
    pend, pend_lo, pend_rows = [], 0, 0

    def flush():
        nonlocal best_rows, best_dist, pend, pend_lo, pend_rows
        if not pend:
            return
        block = np.concatenate(pend) if len(pend) > 1 else pend[0]
        rows, dist, counts = oracle.search_batch(0, block, queries, kk)
        rows = np.where(np.arange(rows.shape[1])[None, :] < counts[:, None], rows + pend_lo, -1)
        dist = np.where(rows >= 0, dist, np.inf).astype(np.float32)
        allr = np.concatenate([best_rows, rows], axis=1)
        alld = np.concatenate([best_dist, dist], axis=1)
        keep_r = np.empty((nq, min(kk, allr.shape[1])), dtype=np.int64)
        keep_d = np.empty(keep_r.shape, dtype=np.float32)
        for i in range(nq):
            rr = np.where(allr[i] >= 0, allr[i], np.iinfo(np.int64).max)
            order = np.lexsort((rr, alld[i]))[:keep_r.shape[1]]
            keep_r[i], keep_d[i] = allr[i][order], alld[i][order]
        best_rows, best_dist = keep_r, keep_d
        pend_lo += pend_rows
        pend, pend_rows = [], 0

    eng.reserve(n)
    for lo, x in _device_corpus(torch, n, dims, dev):
        eng.addBatchDevice(np.arange(lo, lo + x.shape[0], dtype=np.uint64), x)
        pend.append(x.cpu().numpy())
        pend_rows += x.shape[0]
        if pend_rows >= block_rows:
            flush()
    flush()
    counts = np.sum(best_rows >= 0, axis=1)
    return best_rows, best_dist, counts


@pytest.mark.parametrize("n,dims,nq,n_check", [(10_000_000, 768, 1024, 64), (10_000_000, 384, 256, 256)])
def test_batched_full_size_parity_on_one_gpu(wax, n, dims, nq, n_check):
    """BASELINE config 5 at FULL size on one GPU (10M x 768, 1024 queries: the N = 1 point of its scaling curve) and config
    3's batch at the headline's row count (10M x 384, 256 queries): the batched bf16 MFMA path, device-resident, against the
    f64 oracle on the same rows — 64 of the 1024 answers (every 16th query) resp. all 256, id for id and score for score —
    plus bit-identity with the single-query path and zero certificate fallbacks on this corpus."""
    import time
    import torch
    dev = torch.device("cuda", 0)
    k = 10
    queries = oracle.gaussian_unit_queries(nq, dims, seed=77)
    sel = np.arange(0, nq, nq // n_check)
    eng = wax.HIPVectorEngine(dimensions=dims)
    t0 = time.perf_counter()
    rows, dist, counts = _oracle_batch_streaming(eng, torch, n, dims, dev, queries[sel], k + MARGIN)
    t_oracle = time.perf_counter() - t0
    assert eng.count == n
    dq = torch.from_numpy(queries).to(dev)
    out = torch.empty((nq, k, 2), dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    eng.searchBatchHitsDevice(dq.data_ptr(), nq, k, out.data_ptr(), k, st)          # builds the mirror
    q0 = eng.getTuning("onepass_queries")
    t0 = time.perf_counter()
    reps = 3
    for _ in range(reps):
        eng.searchBatchHitsDevice(dq.data_ptr(), nq, k, out.data_ptr(), k, st)
    dt = (time.perf_counter() - t0) / reps
    assert eng.getTuning("onepass_queries") - q0 == reps * nq                        # the one-pass MFMA pipeline served them
    fb = eng.getTuning("batch_fallbacks")
    print(f"\n[{n}x{dims} Q={nq}] {dt * 1e3:.2f} ms/batch (blocking call) = {nq / dt:.0f} q/s, {2 * nq * n * dims / dt / 1e12:.0f} TFLOP/s "
          f"bf16 end to end, fallbacks {fb}; corpus build + streaming oracle for {len(sel)} queries {t_oracle:.1f} s")
    from wax_amd import sharded
    h_ids, h_scores, h_valid = sharded.decode_hits(wax.VectorMetric.cosine, out.cpu().numpy())
    assert np.all(h_valid)
    for j, i in enumerate(sel):
        kk = min(k, int(counts[j]))
        x_scores = oracle.scores_from_distances(0, dist[j, :counts[j]])
        assert_parity(h_ids[i][:kk], h_scores[i][:kk], rows[j, :kk], x_scores[:kk], x_scores, f"{n}x{dims} batched q{i}")
    for i in (0, nq // 2, nq - 1):                                                    # bit-identical to the single-query path
        s_ids, s_scores = eng.searchArrays(queries[i], k)
        assert np.array_equal(h_ids[i], s_ids) and np.array_equal(h_scores[i], s_scores)
    assert fb == 0
    eng.close()


# ---------------------------------------------------------------------------
# the N>1 bench path end to end on one GPU: two / three ranks share GPU 0 and exchange per-shard
# top-k through the host (gloo) — RCCL itself refuses duplicate GPUs; everything else (shard bounds,
# global-row keys, pipelined ShardedSearcher, merge, barriers, max-over-ranks timing) is the code the
# driver runs with --gpus N over RCCL.

def _run_bench(nproc, extra, tmp_path, one_process=False, cpu=False, full=True):
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = (["--rows", "300000", "--steps", "12", "--warmup", "2", "--c5-rows", "300000"] + (["--full"] if full else [])
              + ([] if cpu else ["--no-cpu-baseline"]) + extra)
    env = dict(os.environ)
    env.pop("WAX_HIP_SHARD_MIN_MB", None)          # the bench runs with the library's defaults
    if nproc == 1 or one_process:
        if one_process:
            env["WAX_BENCH_SAME_DEVICE"] = "1"
        cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", str(nproc)] + common
    else:
        env["WAX_BENCH_SAME_DEVICE"] = "1"
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
               "--master-addr", "127.0.0.1", "--master-port", str(29600 + nproc),
               os.path.join(root, "bench.py"), "--gpus", str(nproc), "--exchange", "host"] + common
    detail = os.path.join(str(tmp_path), f"bench_detail_{nproc}_{int(one_process)}_{abs(hash(tuple(extra))) % 10**8}.json")
    cmd += ["--detail-out", detail]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    # the contract: the LAST line of stdout is the one JSON line, and it fits a bounded tail (the driver keeps ~8 KB; round 3's
    # 22 KB line was cut and the round went unrecorded)
    last = out.stdout.strip().splitlines()[-1]
    assert last.startswith("{") and len(last) < 4096, (len(last), last[:200])
    line = json.loads(last)
    full = json.load(open(detail))
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config") + (("roofline",) if "--full" in cmd else ()):
        assert key in line, key
    assert abs(line["value"] - full["value"]) <= 1e-5 * full["value"] and line["config"]["checksum"] == full["config"]["last_result_checksum"]
    if "--full" in cmd:
        assert abs(line["roofline"]["frac"] - full["roofline"]["frac"]) < 1e-5 and line["roofline"]["kernel"] == "wax::scan_kernel"
    assert [x["name"] for x in line.get("secondary", [])] == [x["name"] for x in full.get("secondary", [])]
    full["_line"] = line
    return full


def test_bench_plain_run_is_the_headline_only_and_dumps_its_outputs(wax, tmp_path):
    """Without --full the run times exactly --steps steps and prints the headline: no roofline, CPU baseline or secondaries.
    --dump-outputs writes the last timed step's ids / scores, the very answer the line's checksum was taken over, and a second run
    with the same arguments computes the same arrays."""
    import os
    dumps = [str(tmp_path / f"out{i}") for i in range(2)]
    runs = [_run_bench(1, ["--dump-outputs", d], tmp_path, full=False) for d in dumps]
    run = runs[0]
    assert run["steps"] == 12 and run["warmup"] == 2 and run["dtype"] == "f32" and run["higher_is_better"] is True
    assert abs(run["value"] - 12 / (run["ms_per_step"] * 12e-3)) < 1e-6 * run["value"]
    for key in ("roofline", "cpu_baseline", "secondary"):
        assert key not in run and key not in run["_line"], key
    assert "preflight" not in run["config"]
    ids, scores = (np.load(os.path.join(dumps[0], n + ".npy")) for n in ("ids", "scores"))
    assert ids.dtype == np.float64 and scores.dtype == np.float32 and ids.shape == scores.shape == (10,)
    ck = hashlib.sha256(ids.astype(np.uint64).tobytes() + scores.tobytes()).hexdigest()[:16]
    assert ck == run["config"]["last_result_checksum"]
    assert np.all(np.diff(scores) <= 0) and len(set(ids.tolist())) == 10
    for n in ("ids", "scores"):
        assert np.array_equal(np.load(os.path.join(dumps[1], n + ".npy")), np.load(os.path.join(dumps[0], n + ".npy"))), n
    assert runs[1]["config"]["last_result_checksum"] == ck


def test_bench_contract_and_shard_invariance(wax, tmp_path):
    one = _run_bench(1, ["--secondary", "s10k,s1m,b1m_q256,b1m_q1024,c5_shard,c5_full,clustered_k10,s1250k"], tmp_path)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in one, key
    assert one["n_gpus"] == 1 and one["steps"] == 12 and one["dtype"] == "f32" and one["vs_baseline"] is None
    r = one["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    # frac: per launch, from the calibration pass of the same run (12 chained, event-timed scans); pipeline_frac: the timed region
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9 and r["kernel_launches_timed"] == 12 and r["calibration"]["steps"] == 12
    # the second denominator: the node's own streaming-read rate over the same slab, measured in this run
    assert 1000.0 < r["peak_measured"] < 8000.0 and abs(r["frac_of_measured"] - r["achieved"] / r["peak_measured"]) < 1e-9
    assert one["_line"]["roofline"]["peak_measured"] > 1000.0 and one["_line"]["roofline"]["frac_of_measured"] > 0
    assert abs(r["pipeline_frac"] - 300000 * 384 * 4 * 12 / (one["ms_per_step"] * 12e-3) / 1e9 / 8000.0) < 1e-6
    assert abs(one["value"] - 12 / (one["ms_per_step"] * 12e-3)) < 1e-6 * one["value"]
    assert "300K x 384" in one["metric"] and one["config"]["parallelism"] == "row-shard x1"
    assert one["_line"]["config"]["rccl_ranks"] == 0 and one["_line"]["config"]["parallelism"] == "row-shard x1"
    assert "cpu_baseline" in one["_line"]
    # roofline.traffic: measured in the run itself by a counters-only rocprofv3 child pass over the same corpus (bench.live_traffic)
    assert r["traffic_source"].startswith("measured in this run"), r["traffic_source"]
    assert 0.95 < r["traffic"] / (300000 * 384 * 4) < 1.3, r["traffic"]
    assert one["_line"]["roofline"]["traffic_from"] == "live-pmc" and one["_line"]["roofline"]["traffic"] > 0
    sec = one["secondary"]
    assert [x["name"] for x in sec] == ["s10k", "s1m", "b1m_q256", "b1m_q1024", "c5_shard", "c5_full", "clustered_k10", "s1250k"]
    assert "per-GPU shard at 8 GPUs" in sec[7]["config"] and sec[7]["roofline"]["algorithmic_bytes_per_launch"] == 1_250_000 * 384 * 4
    sec = sec[:7]
    assert all("error" not in x for x in sec), sec
    for x in sec:
        rr = x["roofline"]
        assert x["value"] > 0 and x["ms_per_step"] > 0 and rr["kernel_launches_timed"] >= min(x["steps"], 60)
        assert rr["bound"] in ("hbm", "mfma") and 0 < rr["frac"] < 1.2 and abs(rr["frac"] - rr["achieved"] / rr["peak"]) < 1e-9
    # every BASELINE secondary measures its own roofline.traffic the same way (a counters-only child pass over the same workload)
    for x in sec:
        rr = x["roofline"]
        assert str(rr["traffic_source"]).startswith("measured in this run"), (x["name"], rr["traffic_source"])
        if x["name"] != "s10k":                                     # (a 15 MB store lives in the L2s: far fewer bytes than its size)
            assert 0.9 < rr["traffic"] / rr["algorithmic_bytes_per_launch"] < 1.5, (x["name"], rr["traffic"], rr["algorithmic_bytes_per_launch"])
    assert sec[0]["roofline"]["launches_per_query"] == 1            # 10K rows: the scan kernel's last workgroup merges
    assert sec[1]["roofline"]["launches_per_query"] == 2            # the 1M-row store (1.5 GB) in a stream of scans: the merge launch overlaps the next scan ("merge_overlap_mb")
    # (batches in flight: three for batches of up to 256 queries, two for the 1 024-query ones — bench.secondary_batched)
    assert all(x["pipeline"] == "one-pass" and x["batches_in_flight"] == (3 if x["queries_per_step"] <= 256 else 2) and x["ms_per_step_blocking_call"] > 0
               for x in sec[2:])
    assert all(x["roofline"]["events"] in ("kernel-bound", "bracketed") and x["roofline"]["kernel_avg_ms_bracketed"] > 0 for x in sec[2:])
    assert one["roofline"]["calibration"]["events"] in ("kernel-bound", "bracketed") and one["_line"]["roofline"]["events"] == one["roofline"]["calibration"]["events"]
    assert all(x["certificate_fallbacks"] == 0 for x in sec[2:6])
    assert sec[6]["corpus"] == "clustered" and "ms_per_step_vs_iid_config3" in sec[6]
    print("\n[bench secondary] " + " | ".join(f"{x['name']}: {x['value']:.0f} q/s, {x['ms_per_step']:.3f} ms/step, frac {x['roofline']['frac']:.3f}" for x in sec))
    print(f"[bench clustered k=10] fallbacks/step {sec[6]['certificate_fallbacks_per_step']:.1f}, shared exact passes {sec[6]['shared_exact_passes']}, "
          f"{sec[6]['ms_per_step_vs_iid_config3']:.2f} x the iid batch time")
    c5_one = sec[5]["last_result_checksum"]                          # config 5 (shrunk to 300K rows) on ONE engine
    # the in-timed-region measurement mode (what a rocprofv3 kernel-trace summary is compared with)
    chained = _run_bench(1, ["--no-secondary", "--chain-timed-region", "--traffic", "replay"], tmp_path)
    assert chained["roofline"]["traffic"] is None                    # no committed counter pass exists for this row count
    assert chained["roofline"]["kernel_launches_timed"] == 12 and chained["config"]["last_result_checksum"] == one["config"]["last_result_checksum"]
    two = _run_bench(2, [], tmp_path)
    assert "host (gloo)" in two["config"]["parallelism"]
    # ONE process, three shards inside the library (all on GPU 0 here): same answers again
    lib3 = _run_bench(3, [], tmp_path, one_process=True)
    assert lib3["n_gpus"] == 3 and "wax_hip_engine_create_sharded" in lib3["config"]["parallelism"]
    assert lib3["config"]["last_result_checksum"] == one["config"]["last_result_checksum"]
    assert lib3["roofline"]["kernel_launches_timed"] == 36           # 12 calibration steps x 3 shard scans
    three = _run_bench(3, [], tmp_path)
    assert two["n_gpus"] == 2 and three["n_gpus"] == 3
    assert one["config"]["last_result_checksum"] == two["config"]["last_result_checksum"] \
        == three["config"]["last_result_checksum"]
    # config 5 at N > 1, both launch shapes: ranks + all-gather, and one process on the sharded handle — same hits as one engine
    for run, shape in ((two, "ranks"), (three, "ranks"), (lib3, "handle")):
        c5 = run["secondary"]
        if shape == "handle":
            # the headline store under BOTH exchanges of the handle (round 6; with every shard on one GPU the RCCL one is not taken)
            assert [x["name"] for x in c5[:2]] == ["h_tickets", "h_rccl"] and all("error" not in x for x in c5[:2]), c5[:2]
            assert all(x["last_result_checksum"] == run["config"]["last_result_checksum"] and x["n_gpus"] == 3 for x in c5[:2])
            assert run["config"]["preflight"]["ok"] is True and run["_line"]["config"]["preflight"]["ok"] is True, run["config"]["preflight"]
            assert run["config"]["preflight"]["spread_equals_one_engine"] is True and sum(run["config"]["preflight"]["rows_per_device"]) == 32768
            assert run["config"]["exchange"].startswith("in-library tickets")
            c5 = c5[2:]
        # the rest of the N matrix (1M and 10K rows) on the sharded single-query path, in BOTH launch shapes (round 5: also the
        # one-process shape a driver is most likely to run): same last answer as one engine
        assert [x["name"] for x in c5] == ["s1m", "s10k", "c5"] and all("error" not in x for x in c5), c5
        for x, ref in ((c5[0], sec[1]), (c5[1], sec[0])):
            assert x["n_gpus"] == run["n_gpus"] and x["value"] > 0 and x["last_result_checksum"] == ref["last_result_checksum"], (x, ref)
        # 15 MB are never sharded, in either shape (small-store rule): the store sits on the first GPU, which answers alone
        assert c5[1]["rows_per_gpu"] == [10000] + [0] * (run["n_gpus"] - 1), c5[1]
        if shape == "ranks":
            assert c5[1]["exchange"] == "none (small-store rule)" and isinstance(c5[0]["rows_per_gpu"], int)
        if shape == "handle":
            assert c5[0]["rows_per_gpu"] == [333376, 333376, 333248] and c5[0]["ticket_searches"] > 0, c5[0]       # 1M rows: spread
            assert c5[1]["single_shard_searches"] > 0, c5[1]
            assert [e_["name"] for e_ in run["_line"]["secondary"]] == ["h_tickets", "h_rccl", "s1m", "s10k", "c5"]
            assert run["_line"]["secondary"][3]["rows_per_gpu"] == [10000, 0, 0]
            assert run["config"]["rows_per_gpu"] == [100032, 100032, 99936]
        c5 = c5[2:]
        assert len(c5) == 1 and c5[0]["name"] == "c5" and "error" not in c5[0], c5
        assert c5[0]["n_gpus"] == run["n_gpus"] and c5[0]["queries_per_step"] == 1024 and c5[0]["value"] > 0
        assert c5[0]["last_result_checksum"] == c5_one, (shape, run["n_gpus"])
        assert ("sharded handle" in c5[0]["config"]) == (shape == "handle")
        assert c5[0]["roofline"]["kernel_launches_timed"] >= c5[0]["steps"]


def test_ingest_while_serving_keeps_the_mirror_in_step_row_by_row(wax):
    """`remember -> recall` (MemoryOrchestrator.swift:503-558) interleaves single-frame adds with searches. The reference's
    add is one row copy (MetalVectorEngine.swift:330-357); rounds 1-5 re-converted the WHOLE bf16 mirror after any mutation. 1 000
    single-row adds interleaved with config-3 batches on a 1M-row store: each batch converts the appended row(s) only, answers equal the
    single-query path (which never touches the mirror) on the way and a FRESH engine holding all the rows at the end, and a batch behind an
    add costs a few tens of microseconds more than a batch alone."""
    import time
    import torch
    n, dims, nq, k, adds = 1_000_000, 384, 256, 10, 1000
    dev = torch.device("cuda", 0)
    eng = wax.HIPVectorEngine(dimensions=dims)
    eng.reserve(n + adds)                             # no reallocation inside the loop (growth moves the mirror: tested below)
    for lo, x in _device_corpus(torch, n, dims, dev):
        eng.addBatchDevice(np.arange(lo, lo + x.shape[0], dtype=np.uint64), x)
    queries = oracle.gaussian_unit_queries(nq, dims)
    extra = oracle.gaussian_unit_rows(5_000_000, adds, dims)
    # make some of the new rows matter: copies of queries, slightly perturbed, so that they enter those queries' top-k
    for j in range(0, adds, 7):
        v = queries[j % nq] + 0.02 * extra[j]
        extra[j] = (v / np.linalg.norm(v)).astype(np.float32)
    dq = torch.from_numpy(queries).to(dev)
    out = torch.empty((nq, k, 2), dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def batch():
        eng.searchBatchHitsDevice(dq.data_ptr(), nq, k, out.data_ptr(), k, st)
        torch.cuda.synchronize()

    batch()                                           # builds the mirror: 1M rows converted once
    conv0, rows0 = eng.getTuning("mirror_conversions"), eng.getTuning("mirror_rows_converted")
    assert rows0 == n
    for _ in range(5):
        batch()
    t0 = time.perf_counter()
    for _ in range(100):
        batch()
    t_alone = (time.perf_counter() - t0) / 100
    assert eng.getTuning("mirror_conversions") == conv0          # nothing to convert between two searches
    t_mix = 0.0
    for j in range(adds):
        t1 = time.perf_counter()
        eng.add(10_000_000 + j, extra[j])
        batch()
        t_mix += time.perf_counter() - t1
        if j % 97 == 0:                               # on the way: the batch sees the row added a moment ago, like the single-query path
            hits = out.cpu().numpy()
            for qi in (j % nq, (j * 5 + 3) % nq):
                s_ids, s_scores = eng.searchArrays(queries[qi], k)
                b_ids, b_scores = wax.HIPVectorEngine.hitsToResults(wax.VectorMetric.cosine, hits[qi])
                assert np.array_equal(b_ids, s_ids) and np.array_equal(b_scores, s_scores), (j, qi)
    t_mix /= adds
    assert eng.getTuning("mirror_conversions") - conv0 == adds and eng.getTuning("mirror_rows_converted") - rows0 == adds
    print(f"\n[ingest while serving, 1M x 384, 256 queries] batch alone {t_alone * 1e6:.1f} us, add + batch {t_mix * 1e6:.1f} us: "
          f"+{(t_mix - t_alone) * 1e6:.1f} us per mutation (rounds 1-5: ~500 us of re-conversion at this size)")
    assert t_mix - t_alone < 80e-6, (t_mix, t_alone)
    final = out.cpu().numpy().copy()
    # a fresh engine with all the rows
    fresh = wax.HIPVectorEngine(dimensions=dims)
    fresh.reserve(n + adds)
    for lo, x in _device_corpus(torch, n, dims, dev):
        fresh.addBatchDevice(np.arange(lo, lo + x.shape[0], dtype=np.uint64), x)
    fresh.addBatch(np.arange(adds, dtype=np.uint64) + 10_000_000, extra)
    out2 = torch.empty((nq, k, 2), dtype=torch.int64, device=dev)
    fresh.searchBatchHitsDevice(dq.data_ptr(), nq, k, out2.data_ptr(), k, st)
    torch.cuda.synchronize()
    assert np.array_equal(final, out2.cpu().numpy())
    assert (final[:, :, 1].astype(np.uint64) >= 10_000_000).sum() > 50      # the added rows are really among the answers
    fresh.close()
    eng.close()


def test_mirror_follows_upserts_removals_growth_and_deserialize(wax):
    """The other mutations of SURVEY 8 a9 against the incremental mirror: an upsert converts its row only, a removal moves the mirror's
    tail like the store's (MetalVectorEngine.swift:431-438), capacity growth moves the converted rows instead of converting them again,
    deserialize starts over — every batch equal to the single-query path (which does not use the mirror), for the three metrics."""
    dims, n, nq, k = 128, 40_000, 64, 10
    rng = np.random.default_rng(5)
    for metric in (0, 1, 2):
        corpus = oracle.gaussian_unit_rows(0, n, dims) * (1.0 if metric == 0 else rng.uniform(0.5, 2.0, size=(n, 1)).astype(np.float32))
        eng = wax.HIPVectorEngine(metric=wax.VectorMetric(metric), dimensions=dims)
        eng.addBatch(np.arange(n, dtype=np.uint64), corpus)          # capacity: the reference's doubling from 64
        queries = oracle.gaussian_unit_queries(nq, dims)

        def same_as_single(tag):
            ids, scores, counts = eng.searchBatch(queries, k)
            for qi in range(0, nq, 5):
                s_ids, s_scores = eng.searchArrays(queries[qi], k)
                assert np.array_equal(ids[qi][:counts[qi]], s_ids) and np.array_equal(scores[qi][:counts[qi]], s_scores), (metric, tag, qi)

        same_as_single("built")
        r0 = eng.getTuning("mirror_rows_converted")
        assert r0 == n
        # upserts: rows that become the best hit of a query
        for j in range(20):
            eng.add(int(j * 1999), (queries[j] * (1.0 if metric == 0 else 1.5)).astype(np.float32))
        same_as_single("upserts")
        assert eng.getTuning("mirror_rows_converted") - r0 == 20
        assert eng.searchArrays(queries[3], 1)[0][0] == 3 * 1999
        # removals in front of, between and behind the upserted rows
        r1 = eng.getTuning("mirror_rows_converted")
        for fid in (0, 1999, 17, 39_999, 20_000):
            eng.remove(fid)
        same_as_single("removals")
        assert eng.getTuning("mirror_rows_converted") == r1          # the tail moved; nothing was converted again
        assert eng.count == n - 5
        # an upsert and a removal with no search in between (the dirty row moves with the tail)
        eng.add(int(5 * 1999), (-queries[5]).astype(np.float32))
        eng.remove(int(2 * 1999))
        same_as_single("upsert + removal")
        # growth: appends beyond the capacity reallocate the store; the mirror moves its converted rows
        cap_rows = eng.getTuning("mirror_rows_converted")
        more = oracle.gaussian_unit_rows(900_000, 30_000, dims)
        eng.addBatch(np.arange(30_000, dtype=np.uint64) + 500_000, more)
        same_as_single("growth")
        assert eng.getTuning("mirror_rows_converted") - cap_rows == 30_000, (metric, eng.getTuning("mirror_rows_converted") - cap_rows)
        # deserialize: everything is new
        blob = eng.serialize()
        before = eng.getTuning("mirror_rows_converted")
        eng.deserialize(blob)
        same_as_single("deserialize")
        assert eng.getTuning("mirror_rows_converted") - before == eng.count
        eng.close()


def test_id_table_takes_appends_without_a_rebuild(wax):
    """The id -> row table of the allow-list pre-filter (filter.hip) after appends: only the new rows are inserted; removals and
    deserialize start over; results equal the host-probe path every time."""
    dims, n = 64, 60_000
    corpus = oracle.gaussian_unit_rows(0, n, dims)
    ids = np.arange(n, dtype=np.uint64) * 3 + 7
    eng = make_engine(wax, 0, dims, corpus, ids)
    q = oracle.gaussian_unit_queries(1, dims)[0]
    allow = ids[::2].copy()

    def both(tag):
        eng.setTuning("filter_device_min", 4096)
        d = eng.searchFiltered(q, 20, frameIds=allow)
        eng.setTuning("filter_device_min", -1)
        h = eng.searchFiltered(q, 20, frameIds=allow)
        eng.setTuning("filter_device_min", 4096)
        assert np.array_equal(d[0], h[0]) and np.array_equal(d[1], h[1]), tag
        return d

    both("built")
    assert eng.getTuning("idhash_rows_inserted") == n
    more = oracle.gaussian_unit_rows(700_000, 500, dims)
    more[0] = q
    new_ids = np.arange(500, dtype=np.uint64) + 10_000_000
    eng.addBatch(new_ids, more)
    allow = np.concatenate([allow, new_ids[:100]])
    d = both("appended")
    assert d[0][0] == 10_000_000 and eng.getTuning("idhash_rows_inserted") == n + 500
    eng.add(int(ids[4]), q)                            # upsert: id -> row unchanged
    d = both("upsert")
    assert set(d[0][:2].tolist()) == {10_000_000, int(ids[4])} and eng.getTuning("idhash_rows_inserted") == n + 500
    eng.remove(int(ids[2]))                            # every later row moves: the table starts over
    both("removed")
    assert eng.getTuning("idhash_rows_inserted") == n + 500 + eng.count
    eng.close()


def test_bench_secondaries_carry_cpu_baselines_and_the_general_selection_sizes(wax, tmp_path):
    """Round 6: the 10K and 1M points of the N matrix carry the oracle's CPU scan of the same rows from the same
    run, and the sizes Wax.search(topK: 100 / 334) really asks for (k = 300 / 1000: beyond the fused selection) are bench lines."""
    run = _run_bench(1, ["--secondary", "s10k,s1m,s10m_k300,s1m_k1000", "--traffic", "off", "--cpu-baseline-seconds", "2"], tmp_path, cpu=True)
    sec = {x["name"]: x for x in run["secondary"]}
    assert list(sec) == ["s10k", "s1m", "s10m_k300", "s1m_k1000"] and all("error" not in x for x in sec.values()), sec
    for name in ("s10k", "s1m"):
        cb = sec[name]["cpu_baseline"]
        assert cb["value"] > 0 and cb["cores"] >= 1 and cb["kind"] == "port" and cb["value_1_thread"] > 0 and "rows" in cb["sample"], cb
        assert sec[name]["value"] > cb["value"]                      # (the GPU path is not slower than the host's threads)
    assert sec["s10m_k300"]["top_k"] == 300 and sec["s1m_k1000"]["top_k"] == 1000
    assert "top_k > 192" in sec["s10m_k300"]["roofline"]["note_general_selection"] and sec["s1m_k1000"]["roofline"]["frac"] > 0
    for name in ("s10m_k300", "s1m_k1000"):      # every query through the short selection, none left to the long path
        rf = sec[name]["roofline"]
        assert rf["short_selects"] >= run["steps"] and rf["short_select_failures"] == 0, rf
    line = {x["name"]: x for x in run["_line"]["secondary"]}
    assert line["s10k"]["cpu"]["qps"] > 0 and line["s1m"]["cpu"]["cores"] >= 1 and "cpu" not in line["s1m_k1000"]
    assert run["_line"]["cpu_baseline"]["value"] > 0


def test_search_batch_hits_and_sharded_batch_single_rank(wax):
    from wax_amd import sharded
    dims, n, k = 384, 30000, 10
    corpus = oracle.gaussian_unit_rows(0, n, dims)
    ids = np.arange(n, dtype=np.uint64) + 9
    eng = make_engine(wax, 0, dims, corpus, ids)
    eng.setRowBase(5000)
    queries = oracle.gaussian_unit_queries(40, dims)
    hits, counts = eng.searchBatchHits(queries, k)
    assert hits.shape == (40, k, 2) and np.all(counts == k)
    assert np.all(np.diff(hits[:, :, 0], axis=1) > 0)                       # ascending unique keys
    assert np.all((hits[:, :, 0] & 0xFFFFFFFF) >= 5000)                      # keys carry GLOBAL rows
    d_ids, d_scores, valid = sharded.sharded_search_batch(eng, queries, k, world=1)
    for i, q in enumerate(queries):
        s_ids, s_scores = eng.searchArrays(q, k)
        assert np.array_equal(d_ids[i][valid[i]], s_ids) and np.array_equal(d_scores[i][valid[i]], s_scores)
        assert np.array_equal((hits[i, :, 0] & 0xFFFFFFFF) - 5000 + 9, s_ids.astype(np.int64))
    # two shard engines on one GPU, merged on the host like the N>1 exchange does
    a = make_engine(wax, 0, dims, corpus[:12800], ids[:12800])
    b = make_engine(wax, 0, dims, corpus[12800:], ids[12800:])
    b.setRowBase(12800)
    ha, _ = a.searchBatchHits(queries, k)
    hb, _ = b.searchBatchHits(queries, k)
    merged = sharded.merge_batch_hits_host(np.stack([ha, hb]), k)
    m_ids, m_scores, m_valid = sharded.decode_hits(wax.VectorMetric.cosine, merged)
    eng.setRowBase(0)
    for i, q in enumerate(queries):
        s_ids, s_scores = eng.searchArrays(q, k)
        assert np.array_equal(m_ids[i], s_ids) and np.array_equal(m_scores[i], s_scores)


def test_concurrent_writers_and_readers(wax):
    """The reference's contract (AsyncReadWriteLock, ReadWriteLock.swift:79-156; ConcurrencyStressTests.swift:5-47):
    many concurrent searches, exclusive mutations, nothing torn. Readers run while writers upsert / remove;
    every result a reader sees must be internally consistent (sorted, unique ids, valid scores) and the final
    store must equal the sequentially computed one."""
    dims, n0 = 384, 20000
    corpus = oracle.gaussian_unit_rows(0, n0 + 4000, dims)
    eng = make_engine(wax, 0, dims, corpus[:n0])
    queries = oracle.gaussian_unit_queries(8, dims)
    stop = threading.Event()
    errors = []

    def reader(seed):
        try:
            i = seed
            while not stop.is_set():
                ids, scores = eng.searchArrays(queries[i % 8], 10)
                assert len(ids) == 10 and len(set(ids.tolist())) == 10
                assert np.all(np.diff(scores) <= 0) and np.all(np.isfinite(scores))
                if i % 3 == 0:
                    b_ids, b_scores, counts = eng.searchBatch(queries, 5)
                    assert np.all(counts == 5) and np.all(np.diff(b_scores, axis=1) <= 0)
                i += 1
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    def writer(lo, hi):
        try:
            for i in range(lo, hi, 50):
                eng.addBatch(np.arange(i, i + 50, dtype=np.uint64), corpus[i:i + 50])
                if (i // 50) % 4 == 0:
                    eng.remove(i + 7)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    readers = [threading.Thread(target=reader, args=(s,)) for s in range(4)]
    writers = [threading.Thread(target=writer, args=(n0, n0 + 2000)), threading.Thread(target=writer, args=(n0 + 2000, n0 + 4000))]
    for t in readers + writers:
        t.start()
    for t in writers:
        t.join()
    stop.set()
    for t in readers:
        t.join()
    assert not errors, errors
    removed = {i + 7 for i in range(n0, n0 + 4000, 50) if (i // 50) % 4 == 0}
    assert eng.count == n0 + 4000 - len(removed)
    kind, info, vecs, ids = wax.VectorSerializer.decodeVecSegment(eng.serialize())
    assert set(ids.tolist()) == set(range(n0 + 4000)) - removed
    assert np.array_equal(vecs, corpus[ids.astype(np.int64)])           # every surviving row holds its own vector
    got = eng.searchArrays(queries[0], 10)                                # and search agrees with the oracle on that store
    e_ids, e_scores, _, _ = oracle.search(0, vecs, ids, queries[0], 10)
    assert_parity(got[0], got[1], e_ids, e_scores, ctx="after concurrent mutation")


def test_randomised_shapes_against_oracle(wax):
    """Seeded random sweep over (rows, dims, k, metric, data pattern): every combination through the C ABI
    vs the f64 oracle. Dims mix specialised (fused kernel per dims class), generic float4 and scalar ones."""
    rng = np.random.default_rng(20260220)
    dims_pool = [1, 3, 5, 8, 12, 31, 33, 64, 96, 100, 128, 200, 256, 300, 384, 385, 512, 640, 768, 1000, 1024, 1536]
    for trial in range(48):
        dims = int(rng.choice(dims_pool))
        n = int(rng.choice([1, 2, 5, 17, 63, 64, 65, 100, 511, 777, 1500, 4097, 9000]))
        k = int(rng.choice([1, 2, 3, 10, 24, 30, 64, 65, 100, 192, 193, 300]))
        metric = int(rng.integers(0, 3))
        pattern = rng.choice(["gauss", "gauss_scaled", "ties", "lcg", "dupes"])
        if pattern == "gauss":
            corpus = oracle.gaussian_unit_rows(trial * 100003, n, dims)
        elif pattern == "gauss_scaled":
            corpus = oracle.gaussian_unit_rows(trial * 100003, n, dims) * rng.uniform(0.1, 5.0, (n, 1)).astype(np.float32)
        elif pattern == "ties":
            corpus = oracle.tie_pattern(trial, n, dims)
        elif pattern == "lcg":
            corpus = np.stack([oracle.deterministic_embed(f"doc-{trial}-{i}", dims) for i in range(n)])
        else:
            base = oracle.gaussian_unit_rows(trial, max(1, n // 7 + 1), dims)
            corpus = base[rng.integers(0, base.shape[0], n)]
        ids = rng.permutation(10 * n + 5)[:n].astype(np.uint64)
        q = oracle.gaussian_unit_queries(1, dims, seed=1000 + trial)[0]
        if pattern == "ties":
            q = np.abs(q)
        eng = make_engine(wax, metric, dims, corpus, ids)
        got_ids, got_scores = eng.searchArrays(q, k)
        e_ids, e_scores, _, _ = oracle.search(metric, corpus, ids, q, k)
        x_scores = oracle.search(metric, corpus, ids, q, min(k + MARGIN, 10000))[1]
        ctx = f"trial{trial} n{n} d{dims} k{k} m{metric} {pattern}"
        if pattern in ("ties", "dupes"):
            # exact duplicates: scores must match position by position; ids may only permute among rows that
            # the oracle also scores within 2e-5 of each other (duplicates are bit-identical on the GPU, so
            # there the order is by row — checked exactly in test_exact_ties_resolve_by_ascending_row)
            assert len(got_ids) == len(e_ids), ctx
            assert np.max(np.abs(got_scores.astype(np.float64) - e_scores)) <= 1e-5, ctx
            assert len(set(got_ids.tolist())) == len(got_ids), ctx
        else:
            assert_parity(got_ids, got_scores, e_ids, e_scores, x_scores, ctx)
        eng.close()


def test_pending_embedding_replay_from_wal_payloads(wax):
    """WAL putEmbedding payloads (WALEntryCodec.swift:39-54, golden bytes from
    WALEmbeddingCodecTests.swift:12-33) applied device-side == the same records through addBatch; a bad stream
    changes nothing (decode rules WALEntryCodec.swift:104-129)."""
    w = load_golden("reference_cases.json")["constants"]["put_embedding_wal"]
    enc = wax.HIPVectorEngine.encodePutEmbedding(w["frameId"], w["vector"])
    assert enc.hex() == w["encoded_hex"]
    e2 = wax.HIPVectorEngine(metric=wax.VectorMetric.dot, dimensions=2)
    assert e2.applyPutEmbeddings(enc) == 1 and e2.count == 1
    ids, scores = e2.searchArrays(np.array([1.0, 0.0], np.float32), 1)
    assert ids.tolist() == [1] and scores[0] == pytest.approx(1.0 - 1.0)  # dot score = q.v - 1
    e2.close()

    dims, n = 384, 700
    corpus = oracle.gaussian_unit_rows(5, n, dims)
    ids = (np.arange(n, dtype=np.uint64) * 3 + 11)
    order = np.random.default_rng(2).integers(0, n, 2 * n)   # repeats: later records overwrite earlier ones
    stream = b"".join(wax.HIPVectorEngine.encodePutEmbedding(int(ids[i]), corpus[i] * np.float32(1 + (j % 3)))
                      for j, i in enumerate(order))
    a = wax.HIPVectorEngine(metric=wax.VectorMetric.cosine, dimensions=dims)
    b = wax.HIPVectorEngine(metric=wax.VectorMetric.cosine, dimensions=dims)
    a.addBatch(ids[:50], corpus[:50])
    b.addBatch(ids[:50], corpus[:50])
    assert a.applyPutEmbeddings(stream) == len(order)
    b.addBatch([int(ids[i]) for i in order], np.stack([corpus[i] * np.float32(1 + (j % 3)) for j, i in enumerate(order)]))
    assert a.count == b.count
    assert a.serialize() == b.serialize()
    q = oracle.gaussian_unit_queries(1, dims)[0]
    assert a.search(q, 10) == b.search(q, 10)
    before = a.serialize()
    for bad, exc in ((stream + b"\x04\x01\x02", wax.InvalidToc), (stream + b"\x09" + stream[1:50], wax.InvalidToc),
                     (stream[:-4], wax.InvalidToc), (b"\x01" + stream[1:], wax.InvalidToc),
                     (stream + wax.HIPVectorEngine.encodePutEmbedding(5, np.zeros(3, np.float32)), wax.EncodingError),
                     (b"\x04" + b"\x00" * 8 + (2_000_000).to_bytes(4, "little"), wax.InvalidToc)):
        with pytest.raises(exc):
            a.applyPutEmbeddings(bad)
    assert a.serialize() == before
    assert a.applyPutEmbeddings(b"") == 0
    a.close(); b.close()


def test_filtered_search_reference_case(wax):
    """UnifiedSearchTests.swift:133-158 (filtersAllowResultsBeyondTopK): 4 two-d documents, query [1, 0], topK 2,
    allow-list = the two WORST matches -> exactly those two come back."""
    eng = wax.HIPVectorEngine(metric=wax.VectorMetric.cosine, dimensions=2)
    eng.addBatch([0, 1, 2, 3], np.array([[1.0, 0.0], [0.9, 0.1], [0.1, 0.9], [0.0, 1.0]], np.float32))
    ids, scores = eng.searchFiltered(np.array([1.0, 0.0], np.float32), 2, frameIds=[2, 3])
    assert ids.tolist() == [2, 3]
    full_ids, full_scores = eng.searchArrays(np.array([1.0, 0.0], np.float32), 4)
    assert np.array_equal(scores, full_scores[2:])
    # minScore (UnifiedSearch.swift:1248): `score < minScore` drops the candidate
    ids, scores = eng.searchFiltered(np.array([1.0, 0.0], np.float32), 4, minScore=0.5)
    assert ids.tolist() == [0, 1]
    ids, scores = eng.searchFiltered(np.array([1.0, 0.0], np.float32), 4, frameIds=[3, 1, 99], minScore=0.5)
    assert ids.tolist() == [1]
    assert eng.searchFiltered(np.array([1.0, 0.0], np.float32), 4, frameIds=[])[0].size == 0      # empty list allows nothing
    assert eng.searchFiltered(np.array([1.0, 0.0], np.float32), 4, frameIds=[77, 78])[0].size == 0
    with pytest.raises(wax.EncodingError):
        eng.searchFiltered(np.array([1.0, 0.0, 0.0], np.float32), 2, frameIds=[1])
    eng.close()


@pytest.mark.parametrize("device_min", [4096, 0, -1])
@pytest.mark.parametrize("metric,dims", [(0, 384), (1, 384), (2, 128), (0, 768), (0, 100), (1, 33)])
def test_filtered_search_equals_filtered_full_ranking(wax, metric, dims, device_min):
    """Pre-filter on the device == post-filter of the COMPLETE ranking (what the reference's post-filter would give
    with an unbounded candidateLimit): same ids, and for the specialised dims bit-identical scores. device_min: the
    allow-list length from which ids are resolved by the id -> row table in HBM (0 = always, -1 = host probes only)."""
    n = 6000
    corpus = oracle.gaussian_unit_rows(3, n, dims)
    if metric != 0:
        corpus = corpus * np.linspace(0.5, 2.0, n, dtype=np.float32)[:, None]
    ids = (np.arange(n, dtype=np.uint64) * 7 + 3)
    eng = make_engine(wax, metric, dims, corpus, ids)
    eng.setTuning("filter_device_min", device_min)
    rng = np.random.default_rng(11)
    q = oracle.gaussian_unit_queries(1, dims, seed=21)[0]
    full_ids, full_scores = eng.searchArrays(q, n)           # k = N: the general (radix select) path, complete ranking
    assert len(full_ids) == n
    exact_dims = dims in (128, 384, 768)
    for n_allow, k in [(1, 10), (7, 3), (250, 10), (250, 300), (3000, 30), (n, 10), (n, 250)]:
        allow = rng.permutation(ids)[:n_allow]
        allow_plus = np.concatenate([allow, allow[:3], np.array([10 ** 12], np.uint64)])    # duplicates and an unknown id
        got_ids, got_scores = eng.searchFiltered(q, k, frameIds=allow_plus)
        keep = np.isin(full_ids, allow)
        exp_ids, exp_scores = full_ids[keep][:k], full_scores[keep][:k]
        assert len(got_ids) == len(exp_ids) == min(k, n_allow)
        if exact_dims:
            assert np.array_equal(got_ids, exp_ids) and np.array_equal(got_scores, exp_scores), (n_allow, k)
        else:
            assert np.max(np.abs(got_scores - exp_scores)) <= 1e-6
            assert set(got_ids.tolist()) == set(exp_ids.tolist()) or np.min(np.abs(np.diff(exp_scores))) < 1e-6
        # with a score cut
        cut = float(exp_scores[len(exp_scores) // 2])
        c_ids, c_scores = eng.searchFiltered(q, k, frameIds=allow, minScore=cut)
        assert np.all(c_scores >= cut) and len(c_ids) == int(np.sum(got_scores >= cut))
    # no allow-list: the ordinary search + cut
    o_ids, o_scores = eng.searchArrays(q, 20)
    f_ids, f_scores = eng.searchFiltered(q, 20, minScore=float(o_scores[9]))
    assert np.array_equal(f_ids, o_ids[:len(f_ids)]) and len(f_ids) == int(np.sum(o_scores >= o_scores[9]))
    # after a removal the row list follows the shifted rows
    victim = int(full_ids[0])
    eng.remove(victim)
    g_ids, _ = eng.searchFiltered(q, 5, frameIds=[victim, int(full_ids[1]), int(full_ids[2])])
    assert g_ids.tolist() == [int(full_ids[1]), int(full_ids[2])]
    used = eng.getTuning("filter_device_searches")
    assert (used > 0) if device_min == 0 else (used == 0 if device_min < 0 else used >= 1)
    eng.close()


def test_batch_submit_collect_device_pipeline(wax):
    """wax_hip_search_batch_submit_device / _collect_device: several batches in flight on the engine's workspaces give
    the blocking call's hits bit for bit (different query sets per ticket), uncertified queries are settled at collect, writers are
    refused while the thread holds a batch ticket, a fifth ticket on a four-workspace engine is refused, tickets are
    single-use."""
    import torch
    n, dims, k, nq = 200_000, 384, 10, 256
    corpus = oracle.gaussian_unit_rows(4, n, dims)
    corpus[1000:1064] = corpus[999]                     # a run of duplicates: some certificates fail -> exact path at collect
    eng = make_engine(wax, 0, dims, corpus)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    sets = [oracle.gaussian_unit_queries(nq, dims, seed=40 + i) for i in range(4)]
    sets[1][:8] = corpus[999]                            # queries whose top-k lies inside the duplicate run
    dqs = [torch.from_numpy(q).to(dev) for q in sets]
    ref = []
    for dq in dqs:
        out = torch.empty((nq, k, 2), dtype=torch.int64, device=dev)
        eng.searchBatchHitsDevice(dq.data_ptr(), nq, k, out.data_ptr(), k, st)
        ref.append(out.cpu().numpy())
    outs = [torch.empty((nq, k, 2), dtype=torch.int64, device=dev) for _ in range(4)]
    tickets = [eng.searchBatchSubmitDevice(dqs[i].data_ptr(), nq, k, outs[i].data_ptr(), k, st) for i in range(4)]
    with pytest.raises(wax.WaxError):                # every workspace is taken by this thread's tickets
        eng.searchBatchSubmitDevice(dqs[0].data_ptr(), nq, k, outs[0].data_ptr(), k, st)
    with pytest.raises(wax.WaxError):                # a writer would wait for this thread's own read lock
        eng.add(10 ** 9, corpus[0])
    retries0 = eng.getTuning("batch_retries")
    fallbacks = [eng.searchBatchCollectDevice(t) for t in tickets]
    # the duplicate-run queries cannot be certified by the first finish: they are settled at collect — by the full retry
    # (all survivors re-scored; since round 3 that is enough for a 64-fold tie) or, failing that, by the exact path
    assert fallbacks[0] == 0 and fallbacks[1] + (eng.getTuning("batch_retries") - retries0) >= 1
    for i in range(4):
        assert np.array_equal(outs[i].cpu().numpy(), ref[i]), i
    with pytest.raises(wax.WaxError):
        eng.searchBatchCollectDevice(tickets[0])
    eng.add(10 ** 9, corpus[0])                          # all tickets collected: writers run again
    # a steady two-deep pipeline, then an empty batch and a tiny one (answered at submit time)
    pend = []
    for i in range(12):
        if len(pend) == 2:
            eng.searchBatchCollectDevice(pend.pop(0))
        pend.append(eng.searchBatchSubmitDevice(dqs[i % 4].data_ptr(), nq, k, outs[i % 2].data_ptr(), k, st))
    for t in pend:
        eng.searchBatchCollectDevice(t)
    assert eng.searchBatchCollectDevice(eng.searchBatchSubmitDevice(dqs[0].data_ptr(), 0, k, outs[0].data_ptr(), k, st)) == 0
    t = eng.searchBatchSubmitDevice(dqs[0].data_ptr(), 1, k, outs[0].data_ptr(), k, st)
    eng.searchBatchCollectDevice(t)
    one = outs[0].cpu().numpy()[0]
    ids1, _ = eng.searchArrays(sets[0][0], k)
    assert np.array_equal(one[:, 1].view(np.uint64), ids1)
    eng.close()


def test_filtered_search_long_allow_list_on_device(wax):
    """A long allow-list (FrameFilter.frameIds with 10^5 ids) is resolved by the id -> row table in HBM: same answer as
    the host-probe path bit for bit, also after removals (rows shift), appends and an upsert; concurrent callers each
    take their own workspace."""
    n, dims = 300_000, 128
    corpus = oracle.gaussian_unit_rows(5, n + 1000, dims)
    ids = np.arange(n + 1000, dtype=np.uint64) * 3 + 11
    eng = make_engine(wax, 0, dims, corpus[:n], ids[:n])
    rng = np.random.default_rng(2)
    queries = oracle.gaussian_unit_queries(6, dims, seed=8)

    def both(allow, k, q):
        eng.setTuning("filter_device_min", -1)
        h = eng.searchFiltered(q, k, frameIds=allow)
        eng.setTuning("filter_device_min", 4096)
        before = eng.getTuning("filter_device_searches")
        d = eng.searchFiltered(q, k, frameIds=allow)
        assert eng.getTuning("filter_device_searches") == before + (1 if len(allow) >= 4096 else 0)
        assert np.array_equal(h[0], d[0]) and np.array_equal(h[1], d[1])
        return d

    allow = np.concatenate([rng.permutation(ids[:n])[:100_000], np.array([1, 2, 10 ** 15], np.uint64)])   # + unknown ids
    allow = np.concatenate([allow, allow[:5000]])                                                         # + duplicates
    got_ids, got_scores = both(allow, 50, queries[0])
    assert len(got_ids) == 50 and np.all(np.isin(got_ids, allow)) and np.all(np.diff(got_scores) <= 0)
    # against the complete ranking
    full_ids, full_scores = eng.searchArrays(queries[0], 10_000)
    keep = np.isin(full_ids, allow)
    assert np.array_equal(got_ids[:int(min(50, keep.sum()))], full_ids[keep][:50])
    # every id allowed: the filtered search IS the plain search
    a_ids, a_scores = both(ids[:n], 25, queries[1])
    p_ids, p_scores = eng.searchArrays(queries[1], 25)
    assert np.array_equal(a_ids, p_ids) and np.array_equal(a_scores, p_scores)
    # mutations invalidate the table: removal (rows shift down), append, upsert in place
    for victim in (int(got_ids[0]), int(ids[0]), int(ids[n - 1])):
        eng.remove(victim)
    eng.addBatch(ids[n:n + 1000], corpus[n:n + 1000])
    eng.add(int(ids[77]), corpus[n + 5])
    allow2 = np.concatenate([allow, ids[n:n + 500]])
    r_ids, _ = both(allow2, 50, queries[0])
    assert int(got_ids[0]) not in r_ids.tolist()
    # concurrent filtered searches (pooled workspaces, one stream each)
    expect = [both(allow2, 20, q) for q in queries]
    errors = []

    def worker(i):
        try:
            for _ in range(5):
                g = eng.searchFiltered(queries[i], 20, frameIds=allow2)
                assert np.array_equal(g[0], expect[i][0]) and np.array_equal(g[1], expect[i][1])
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(len(queries))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    eng.close()


@pytest.mark.parametrize("dims", [384, 128, 768, 256, 512])
def test_batch_gemm_variants_agree(wax, dims):
    """Every GEMM behind the batched path — the LDS-tiled kernel (batch_rega 0), the register-resident-queries kernel with a
    workgroup barrier per tile (1, the default since round 6) and with the split barrier (5), with and without the pace gate — gives the
    single-query answers bit for bit, over several slab schedules of the slab pipeline and through the one-pass pipeline.
    (Round 5 replaced four register-resident kernels and a dozen build variants by this one; what they measured is in profiles/HISTORY.md.)"""
    n = 150_000
    corpus = oracle.gaussian_unit_rows(9, n, dims)
    eng = make_engine(wax, 0, dims, corpus)
    queries = oracle.gaussian_unit_queries(300, dims, seed=31)
    ref = None
    for onepass, rega, growth, *dbg in [(0, 1, 8), (0, 1, 3), (0, 0, 8), (0, 0, 3), (1, 1, 8), (1, 5, 8), (0, 5, 3), (0, 5, 16), (1, 5, 8, 4096), (1, 0, 8)]:
        eng.setTuning("batch_debug", dbg[0] if dbg else 0)
        eng.setTuning("batch_onepass", onepass)
        eng.setTuning("batch_rega", rega)
        eng.setTuning("batch_growth", growth)
        before, before1 = eng.getTuning("batch_queries"), eng.getTuning("onepass_queries")
        ids, scores, counts = eng.searchBatch(queries, 10)
        assert eng.getTuning("batch_queries") - before == 300
        assert eng.getTuning("onepass_queries") - before1 == (300 if onepass else 0)
        if ref is None:
            ref = (ids, scores, counts)
            for i in (0, 1, 150, 299):
                s_ids, s_scores = eng.searchArrays(queries[i], 10)
                assert np.array_equal(ids[i], s_ids) and np.array_equal(scores[i], s_scores)
        else:
            assert np.array_equal(ids, ref[0]) and np.array_equal(scores, ref[1]) and np.array_equal(counts, ref[2])
    eng.setTuning("batch_debug", 0)
    assert eng.getTuning("batch_fallbacks") <= 80
    eng.close()


@pytest.mark.parametrize("dims,rega,dbg", [(384, 5, 0), (768, 5, 0), (128, 5, 4096)])
def test_split_barrier_timeout_is_fail_safe(wax, dims, rega, dbg):
    """The filtering GEMM synchronises its tiles through an LDS counter with BOUNDED spins (a protocol error must not hang the GPU).
    A wave that gives up must not produce a silent wrong answer: its workgroup reports every one of its queries as overflowed and
    those queries are answered by the exact path. "batch_debug" bit 14 makes one wave of workgroup 1 pretend it timed out."""
    n = 160_000
    corpus = oracle.gaussian_unit_rows(21, n, dims)
    eng = make_engine(wax, 0, dims, corpus)
    queries = oracle.gaussian_unit_queries(300, dims, seed=5)
    eng.setTuning("batch_rega", rega)
    eng.setTuning("batch_debug", dbg)
    ref = eng.searchBatch(queries, 10)
    f0 = eng.getTuning("batch_fallbacks")
    eng.setTuning("batch_debug", 16384 | dbg)
    got = eng.searchBatch(queries, 10)
    eng.setTuning("batch_debug", 0)
    hit = eng.getTuning("batch_fallbacks") - f0
    assert hit >= 256, hit                                   # one workgroup's 256 queries took the exact path
    for a, b in zip(got, ref):
        assert np.array_equal(a, b)
    eng.close()


def test_batch_randomised_soak(wax):
    """Seeded random sweep of the batched path: ragged corpus sizes (partial last tiles of every GEMM variant), query
    counts that are not multiples of the 128/256-query groups, k up to the MFMA limit, every staging mode and several
    slab schedules — each batch must equal the single-query answers bit for bit."""
    rng = np.random.default_rng(424242)
    for trial in range(20):
        dims = int(rng.choice([128, 256, 384, 512, 768, 768, 384, 64, 192]))
        metric = int(rng.choice([0, 0, 1, 2])) if dims in (64, 192) else int(rng.choice([0, 0, 1]))
        n = int(rng.integers(90, 70000))
        nq = int(rng.integers(16, 400))
        k = int(rng.choice([1, 5, 10, 30, 80]))
        corpus = oracle.gaussian_unit_rows(1000 + trial, n, dims)
        if metric != 0:
            corpus = corpus * rng.uniform(0.5, 1.5, (n, 1)).astype(np.float32)
        eng = make_engine(wax, metric, dims, corpus)
        eng.setTuning("batch_rega", int(rng.choice([1, 5, 5, 0])))
        eng.setTuning("batch_growth", int(rng.choice([3, 8, 16])))
        eng.setTuning("batch_first", int(rng.choice([512, 2048])))
        queries = oracle.gaussian_unit_queries(nq, dims, seed=500 + trial)
        before = eng.getTuning("batch_queries")
        ids, scores, counts = eng.searchBatch(queries, k)
        assert eng.getTuning("batch_queries") - before == nq, (trial, dims, n, nq, k)
        for i in rng.permutation(nq)[:40]:
            s_ids, s_scores = eng.searchArrays(queries[i], k)
            ctx = (trial, dims, metric, n, nq, k, int(i))
            assert counts[i] == len(s_ids), ctx
            assert np.array_equal(ids[i, :counts[i]], s_ids), ctx
            assert np.array_equal(scores[i, :counts[i]], s_scores), ctx
        eng.close()


def test_merge_batch_hits_device_equals_host_merge(wax):
    """The sharded batched exchange (config 5): [shards][nq][k] gathered hits -> [nq][k], one workgroup per query,
    must equal the numpy host merge and the single-engine answer."""
    import torch
    from wax_amd import sharded
    dims, k, nq = 384, 10, 130
    corpus = oracle.gaussian_unit_rows(0, 30000, dims)
    ids = np.arange(30000, dtype=np.uint64) + 5
    bounds = [0, 9984, 20096, 30000]
    queries = oracle.gaussian_unit_queries(nq, dims, seed=77)
    shard_hits = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        e = make_engine(wax, 0, dims, corpus[lo:hi], ids[lo:hi])
        e.setRowBase(lo)
        h, _ = e.searchBatchHits(queries, k)
        shard_hits.append(h)
        e.close()
    gathered = np.stack(shard_hits)                                   # [3][nq][k][2]
    host = sharded.merge_batch_hits_host(gathered, k)
    dev = torch.device("cuda", 0)
    g = torch.from_numpy(np.ascontiguousarray(gathered)).to(dev)
    out = torch.empty((nq, k, 2), dtype=torch.int64, device=dev)
    wax.HIPVectorEngine.mergeBatchHitsDevice(g.data_ptr(), 3, nq, k, k, out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), host)
    whole = make_engine(wax, 0, dims, corpus, ids)
    w_hits, _ = whole.searchBatchHits(queries, k)
    assert np.array_equal(out.cpu().numpy(), w_hits)
    # lists padded with KEY_PAD (a shard smaller than k) and k_in > k
    padded = np.concatenate([gathered, np.full((3, nq, 3, 2), -1, dtype=np.int64)], axis=2)
    padded[:, :, k:, 0] = sharded.KEY_PAD
    g2 = torch.from_numpy(np.ascontiguousarray(padded)).to(dev)
    out2 = torch.empty((nq, 4, 2), dtype=torch.int64, device=dev)
    wax.HIPVectorEngine.mergeBatchHitsDevice(g2.data_ptr(), 3, nq, k + 3, 4, out2.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(out2.cpu().numpy(), host[:, :4])
    whole.close()


def test_mixed_entry_points_under_concurrency(wax):
    """Every read entry point at once — single search, submit/collect with several tickets outstanding, batched
    (MFMA) search, filtered search, serialize — against a writer that keeps appending: no deadlock (the readers hold
    tickets while the writer queues for the exclusive lock), no torn result."""
    dims, n0 = 384, 30000
    corpus = oracle.gaussian_unit_rows(0, n0 + 3000, dims)
    eng = make_engine(wax, 0, dims, corpus[:n0])
    eng.setTuning("slots", 4)
    queries = oracle.gaussian_unit_queries(64, dims, seed=3)
    stop = threading.Event()
    errors = []

    def guard(fn):
        def run():
            try:
                while not stop.is_set():
                    fn()
            except Exception as e:  # noqa: BLE001
                errors.append(e)
        return run

    def single():
        ids, scores = eng.searchArrays(queries[1], 10)
        assert len(ids) == 10 and np.all(np.diff(scores) <= 0)

    def pipelined():
        tickets = [eng.submit(queries[i], 10) for i in range(3)]
        for t in tickets:
            ids, scores = eng.collect(t, 10)
            assert len(set(ids.tolist())) == 10

    def batched():
        ids, scores, counts = eng.searchBatch(queries, 10)
        assert np.all(counts == 10) and np.all(np.diff(scores, axis=1) <= 0)

    def filtered():
        allow = np.arange(0, 20000, 7, dtype=np.uint64)
        ids, scores = eng.searchFiltered(queries[2], 10, frameIds=allow, minScore=-1.0)
        assert len(ids) == 10 and np.all(ids % 7 == 0)

    def snapshot():
        blob = eng.serialize()
        assert blob[:4] == b"MV2V"

    def writer():
        try:
            for i in range(n0, n0 + 3000, 100):
                eng.addBatch(np.arange(i, i + 100, dtype=np.uint64), corpus[i:i + 100])
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    readers = [threading.Thread(target=guard(f)) for f in (single, pipelined, batched, filtered, snapshot, pipelined)]
    w = threading.Thread(target=writer)
    for t in readers:
        t.start()
    w.start()
    w.join(timeout=60)
    stop.set()
    for t in readers:
        t.join(timeout=10)
    assert not w.is_alive() and not any(t.is_alive() for t in readers), "deadlock"
    assert not errors, errors
    assert eng.count == n0 + 3000
    got = eng.searchArrays(queries[0], 10)
    e_ids, e_scores, _, _ = oracle.search(0, corpus, np.arange(n0 + 3000, dtype=np.uint64), queries[0], 10)
    assert_parity(got[0], got[1], e_ids, e_scores, ctx="after mixed concurrency")
    eng.close()


def test_staged_single_frame_appends(wax):
    """add(frameId:vector:) stages the row on the host and the next reader uploads everything added since (the
    discrete-memory analogue of the reference's unified-memory append, MetalVectorEngine.swift:330-357). Interleave
    appends, upserts of staged and of already-uploaded rows, removals, batch adds, capacity growth, serialize and every
    kind of reader; the store must always equal the sequentially built one."""
    dims = 384
    rng = np.random.default_rng(5)
    pool = oracle.gaussian_unit_rows(77, 9000, dims)
    eng = wax.HIPVectorEngine(metric=wax.VectorMetric.cosine, dimensions=dims)
    model_ids, model_rows = [], {}

    def model_add(i, v):
        if i not in model_rows:
            model_ids.append(i)
        model_rows[i] = v

    def check(ctx):
        kind, info, vecs, ids = wax.VectorSerializer.decodeVecSegment(eng.serialize())
        assert ids.tolist() == model_ids, ctx
        assert np.array_equal(vecs, np.stack([model_rows[i] for i in model_ids])), ctx
        q = pool[rng.integers(0, 9000)]
        got = eng.searchArrays(q, 5)
        e_ids, e_scores, _, _ = oracle.search(0, vecs, ids, q, 5)
        assert_parity(got[0], got[1], e_ids, e_scores, ctx=ctx)

    step = 0
    for i in range(300):                                   # appends crossing several capacity doublings (64, 128, 256)
        eng.add(i, pool[step]); model_add(i, pool[step]); step += 1
    eng.add(5, pool[step]); model_add(5, pool[step]); step += 1            # upsert of a STAGED row
    check("after staged appends")
    eng.add(7, pool[step]); model_add(7, pool[step]); step += 1            # upsert of an UPLOADED row
    for i in range(300, 320):
        eng.add(i, pool[step]); model_add(i, pool[step]); step += 1
    eng.remove(310); model_ids.remove(310); del model_rows[310]           # removal while rows are staged
    eng.remove(3); model_ids.remove(3); del model_rows[3]
    check("after remove with staged rows")
    for i in range(320, 330):
        eng.add(i, pool[step]); model_add(i, pool[step]); step += 1
    b_ids = list(range(1000, 1100)) + [321, 2]             # batch add with staged rows in front, touching staged / uploaded ids
    b_rows = pool[step:step + len(b_ids)]; step += len(b_ids)
    eng.addBatch(b_ids, b_rows)
    for i, v in zip(b_ids, b_rows):
        model_add(i, v)
    for i in range(330, 340):
        eng.add(i, pool[step]); model_add(i, pool[step]); step += 1
    ids_b, scores_b, counts_b = eng.searchBatch(pool[:40], 3)             # batched reader flushes too
    f_ids, _ = eng.searchFiltered(pool[0], 3, frameIds=[339, 338, 1000])  # and the filtered one
    assert set(f_ids.tolist()) == {339, 338, 1000}
    check("after batch add")
    blob = eng.serialize()
    for i in range(5000, 5010):
        eng.add(i, pool[step]); step += 1                  # staged rows ...
    eng.deserialize(blob)                                  # ... are dropped with the store they belonged to
    check("after deserialize")
    many = 8 * 1024 * 1024 // (dims * 4) + 300             # more single adds than the staging area holds
    base = 100000
    for j in range(many):
        v = pool[j % 9000]
        eng.add(base + j, v); model_add(base + j, v)
    check("after overflowing the staging area")
    eng.close()


@pytest.mark.parametrize("metric", [0, 1, 2])
def test_batch_path_special_values(wax, metric):
    """Zero rows, NaN / inf rows, tiny-norm rows and a zero query through the batched (MFMA) path: the answers must
    still equal the single-query path's (which drops non-finite distances on the host, MetalVectorEngine.swift:597) —
    either certified or via the exact fallback, never approximated."""
    dims, n = 384, 20000
    corpus = oracle.gaussian_unit_rows(0, n, dims)
    if metric != 0:
        corpus = corpus * np.linspace(0.5, 2.0, n, dtype=np.float32)[:, None]
    corpus[5] = 0.0
    corpus[7, 3] = np.nan
    corpus[9] *= np.float32(1e-4)
    corpus[11, 0] = np.inf
    corpus[13, 1] = -np.inf
    corpus[15] = corpus[14]                         # an exact duplicate pair
    eng = make_engine(wax, metric, dims, corpus)
    queries = oracle.gaussian_unit_queries(40, dims, seed=8)
    queries[3] = 0.0                                # zero query
    queries[4] = corpus[14]                         # hits the duplicate pair exactly
    queries[5] = corpus[9] * np.float32(1e4)        # the tiny-norm row's direction
    before = eng.getTuning("batch_queries")
    ids, scores, counts = eng.searchBatch(queries, 10)
    assert eng.getTuning("batch_queries") - before == 40
    for i, q in enumerate(queries):
        s_ids, s_scores = eng.searchArrays(q, 10)
        assert counts[i] == len(s_ids), (metric, i, counts[i], len(s_ids))
        assert np.array_equal(ids[i, :counts[i]], s_ids), (metric, i, ids[i, :counts[i]], s_ids)
        assert np.array_equal(scores[i, :counts[i]], s_scores), (metric, i)
        assert np.all(np.isfinite(scores[i, :counts[i]]))
    eng.close()


# ---------------------------------------------------------------------------
# ABI v2: explicit output capacities, ticket ownership, shard scratch reuse

def test_output_capacity_is_never_exceeded(wax):
    """The library writes at most `capacity` entries whatever top_k and the row count are (a concurrent add between
    the caller's sizing and the search must not overflow the caller's arrays): guard words stay intact."""
    import ctypes
    from wax_amd import _abi
    dims, n = 64, 500
    corpus = oracle.gaussian_unit_rows(0, n, dims)
    eng = make_engine(wax, 0, dims, corpus)
    lib = _abi.lib()
    q = np.ascontiguousarray(oracle.gaussian_unit_queries(1, dims)[0])
    qp = q.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    full_ids, full_scores = eng.searchArrays(q, 300)
    for top_k, cap in [(10, 3), (300, 7), (10000, 1), (5, 0), (10, 10)]:
        ids = np.full(cap + 4, 0xDEADBEEF, dtype=np.uint64)
        scores = np.full(cap + 4, -7.0, dtype=np.float32)
        got = ctypes.c_uint32(99)
        rc = lib.wax_hip_search(eng._h, qp, dims, top_k, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                scores.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), cap, ctypes.byref(got))
        assert rc == 0 and got.value == min(cap, top_k, n)
        assert np.array_equal(ids[:got.value], full_ids[:got.value]) and np.array_equal(scores[:got.value], full_scores[:got.value])
        assert np.all(ids[cap:] == 0xDEADBEEF) and np.all(scores[cap:] == -7.0)
        # ticket form: collect with a smaller capacity than the submit's top_k
        t = ctypes.c_uint64(0)
        assert lib.wax_hip_search_submit(eng._h, qp, dims, top_k, ctypes.byref(t)) == 0
        ids[:] = 0xDEADBEEF
        assert lib.wax_hip_search_collect(eng._h, t.value, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                          scores.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), cap, ctypes.byref(got)) == 0
        assert got.value == min(cap, top_k, n) and np.all(ids[cap:] == 0xDEADBEEF)
    # batch forms: the row stride is the caller's, rows are padded, nothing is written past nq * stride
    qs = np.ascontiguousarray(oracle.gaussian_unit_queries(20, dims))
    for top_k, stride in [(10, 4), (10, 16), (700, 5)]:
        hits = np.full((20 * stride + 3, 2), 12345, dtype=np.int64)
        counts = np.zeros(20, dtype=np.uint32)
        rc = lib.wax_hip_search_batch_hits(eng._h, qs.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 20, dims, top_k,
                                           hits.ctypes.data_as(ctypes.POINTER(_abi.Hit)), stride,
                                           counts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
        assert rc == 0 and np.all(counts == min(stride, top_k, n)) and np.all(hits[20 * stride:] == 12345)
        ids = np.full(20 * stride + 3, 0xDEADBEEF, dtype=np.uint64)
        scores = np.full(20 * stride + 3, -7.0, dtype=np.float32)
        rc = lib.wax_hip_search_batch(eng._h, qs.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 20, dims, top_k,
                                      ids.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                      scores.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), stride,
                                      counts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
        assert rc == 0 and np.all(ids[20 * stride:] == 0xDEADBEEF)
        for i in range(20):
            e_ids, _ = eng.searchArrays(qs[i], top_k)
            m = min(stride, len(e_ids))
            assert counts[i] == m and np.array_equal(ids[i * stride:i * stride + m], e_ids[:m])
    assert lib.wax_hip_result_capacity(-5) == 1 and lib.wax_hip_result_capacity(123) == 123


def test_search_while_index_grows_past_the_sized_count(wax):
    """A small, still-ingesting index searched with a large topK while another thread adds rows (the
    result count is read under the lock inside the library; the wrappers size by topK)."""
    dims = 32
    eng = wax.HIPVectorEngine(dimensions=dims)
    rows = oracle.gaussian_unit_rows(0, 3000, dims)
    eng.addBatch(np.arange(5, dtype=np.uint64), rows[:5])
    stop = threading.Event()
    errors = []

    def writer():
        i = 5
        while not stop.is_set() and i < 3000:
            eng.add(i, rows[i])
            i += 1

    def reader():
        try:
            q = rows[1]
            while not stop.is_set():
                ids, scores = eng.searchArrays(q, 1000)
                assert 5 <= len(ids) <= 1000 and ids[0] == 1 and np.all(np.diff(scores) <= 0)
                b_ids, b_scores, counts = eng.searchBatch(rows[:3], 1000)
                assert counts[0] >= 1 and b_ids[1, 0] == 1
        except Exception as ex:  # noqa: BLE001
            errors.append(ex)

    ts = [threading.Thread(target=writer)] + [threading.Thread(target=reader) for _ in range(3)]
    for t in ts:
        t.start()
    ts[0].join()
    stop.set()
    for t in ts[1:]:
        t.join()
    assert not errors, errors
    assert eng.count == 3000


def test_writer_with_outstanding_ticket_is_refused_not_deadlocked(wax):
    dims = 48
    corpus = oracle.gaussian_unit_rows(0, 2000, dims)
    eng = make_engine(wax, 0, dims, corpus)
    blob = make_engine(wax, 0, dims, corpus[:10]).serialize()   # a well-formed segment (validated before the lock)
    t = eng.submit(corpus[3], 5)
    for name, call in [("add", lambda: eng.add(99999, corpus[0])), ("remove", lambda: eng.remove(3)),
                       ("reserve", lambda: eng.reserve(10000)), ("setRowBase", lambda: eng.setRowBase(5)),
                       ("deserialize", lambda: eng.deserialize(blob))]:
        with pytest.raises(wax.EncodingError) as ei:
            call()
        assert "collect outstanding search tickets first" in str(ei.value), name
    ids, _ = eng.collect(t, 5)
    assert ids[0] == 3
    eng.add(99999, corpus[0])                              # fine once the ticket is collected
    assert eng.count == 2001
    # a ticket collected by ANOTHER thread releases the submitter: it can write again and does not leak "holding"
    t2 = eng.submit(corpus[7], 5)
    got = []
    th = threading.Thread(target=lambda: got.append(eng.collect(t2, 5)))
    th.start()
    th.join()
    assert got[0][0][0] == 7
    eng.remove(99999)
    assert eng.count == 2000


def test_shard_scratch_ring_is_safe_beyond_its_depth(wax):
    """More searches in flight than the library's shard scratch ring has entries (entry reuse is now
    ordered by a per-entry completion event), and a writer right behind in-flight shard searches."""
    import torch
    from wax_amd import sharded
    dims, n, k = 384, 200_000, 10
    corpus = oracle.gaussian_unit_rows(0, n, dims)
    eng = make_engine(wax, 0, dims, corpus)
    queries = oracle.gaussian_unit_queries(40, dims)
    expect = [eng.searchArrays(q, k) for q in queries]
    s = sharded.ShardedSearcher(eng, 0, 1, k, depth=24, n_streams=3)
    out = []
    for i, q in enumerate(queries):
        if len(s.inflight) >= 24:
            out.append(s.collect())
        s.submit(q)
    while s.inflight:
        out.append(s.collect())
    for (ids, scores), (e_ids, e_scores) in zip(out, expect):
        assert np.array_equal(ids, e_ids) and np.array_equal(scores, e_scores)
    # writer immediately after un-synchronised shard searches: it must wait for them (results stay those of the old rows)
    for q in queries[:6]:
        s.submit(q)
    eng.remove(int(expect[0][0][0]))
    got = [s.collect() for _ in range(6)]
    for (ids, scores), (e_ids, e_scores) in zip(got, expect[:6]):
        assert np.array_equal(ids, e_ids) and np.array_equal(scores, e_scores)
    torch.cuda.synchronize()
    ids, _ = eng.searchArrays(queries[0], k)
    assert int(expect[0][0][0]) not in ids


# ---------------------------------------------------------------------------
# one-pass batched pipeline (sampled thresholds -> one filtering GEMM -> fused finish) and the device-resident entry point

@pytest.mark.parametrize("metric,dims", [(0, 384), (1, 384), (0, 128), (0, 768), (1, 768), (0, 256), (0, 512),
                                         (2, 384), (2, 768), (0, 1024), (1, 1536), (2, 1024), (0, 192), (2, 64)])
def test_batch_onepass_pipeline_is_exact(wax, metric, dims):
    """Stores of >= 1024 GEMM tiles take the one-pass pipeline: every answer equals the single-query path bit for bit
    (ids, scores, counts), for k from 1 to 300 (k' = 2k + 32 up to 632: the real caller's candidateLimit range,
    UnifiedSearch.swift:1195-1200), with a row_base, with a query count that is not a multiple of 256; spot-checked
    against the f64 oracle. Round 3: L2 at every dimension and cosine / dot at the other multiples of 64 (1024, 1536, 192)
    take the same pipeline on the LDS-tiled GEMM (sampling variant + one counted survivor list per query)."""
    n = 90_000 if dims < 768 else (50_000 if (dims == 768 and metric != 2) else 70_000)   # >= 1024 tiles of the serving GEMM kernel
    corpus = oracle.gaussian_unit_rows(3, n, dims)
    if metric != 0:
        corpus = corpus * np.linspace(0.6, 1.8, n, dtype=np.float32)[:, None]
    ids = np.arange(n, dtype=np.uint64) * 3 + 11
    eng = make_engine(wax, metric, dims, corpus, ids)
    eng.setRowBase(4096)
    queries = oracle.gaussian_unit_queries(301, dims, seed=77)
    rng = np.random.default_rng(5)
    for k in (10, 1, 80, 150, 300):
        before, before1 = eng.getTuning("batch_queries"), eng.getTuning("onepass_queries")
        b_ids, b_scores, counts = eng.searchBatch(queries, k)
        assert eng.getTuning("batch_queries") - before == 301 and eng.getTuning("onepass_queries") - before1 == 301, k
        for i in list(rng.permutation(301)[:24]) + [0, 300]:
            s_ids, s_scores = eng.searchArrays(queries[i], k)
            assert counts[i] == len(s_ids) == k
            assert np.array_equal(b_ids[i, :k], s_ids), (metric, dims, k, i)
            assert np.array_equal(b_scores[i, :k], s_scores), (metric, dims, k, i)
        for i in (7, 123):
            e_ids, e_scores, _, _ = oracle.search(metric, corpus, ids, queries[i], k)
            x = oracle.search(metric, corpus, ids, queries[i], k + MARGIN)[1]
            assert_parity(b_ids[i, :k], b_scores[i, :k], e_ids, e_scores, x, f"onepass m{metric} d{dims} k{k} q{i}")
    # the split tile barrier instead of the workgroup barrier (the default) gives the same answers
    ref_ids, ref_scores, _ = eng.searchBatch(queries, 30)
    eng.setTuning("batch_rega", 5)
    w_ids, w_scores, _ = eng.searchBatch(queries, 30)
    eng.setTuning("batch_rega", 1)
    assert np.array_equal(ref_ids, w_ids) and np.array_equal(ref_scores, w_scores)
    fb = eng.getTuning("batch_fallbacks")
    print(f"\n[onepass m{metric} d{dims}] fallbacks {fb} of {7 * 301}")
    if metric == 0:
        assert fb <= (30 if dims in (128, 256, 384, 512, 768) else 80)   # (the LDS-tiled kernel samples 128-row tiles: coarser thresholds)
    # the slab pipeline gives the same answers where it applies (k <= 80)
    o_ids, o_scores, _ = eng.searchBatch(queries, 10)
    eng.setTuning("batch_onepass", 0)
    before1 = eng.getTuning("onepass_queries")
    s_ids, s_scores, _ = eng.searchBatch(queries, 10)
    assert eng.getTuning("onepass_queries") == before1
    assert np.array_equal(o_ids, s_ids) and np.array_equal(o_scores, s_scores)
    eng.close()


def test_batch_onepass_adversarial_corpora(wax):
    """Where the sampled threshold cannot certify — exact duplicates (period-256 tie corpus), a clustered corpus whose
    near neighbours sit in one contiguous block, a zero query, NaN / inf rows — the answer still equals the single-query
    path (certificate refuses, exact path answers), and thresholds tuned far too tight or too loose change nothing."""
    dims = 128
    n = 100_000
    ties = oracle.tie_pattern(0, n, dims)
    eng = make_engine(wax, 0, dims, ties)
    queries = np.abs(oracle.gaussian_unit_queries(40, dims))
    before1 = eng.getTuning("onepass_queries")
    _batch_vs_single(eng, queries, 24)
    assert eng.getTuning("onepass_queries") - before1 == 40 and eng.getTuning("batch_fallbacks") > 0
    eng.close()
    # clustered: rows [40000, 40600) are tight around one direction, queries aim at it; special values sprinkled in
    corpus = oracle.gaussian_unit_rows(1, n, dims)
    centre = oracle.gaussian_unit_queries(1, dims, seed=99)[0]
    noise = oracle.gaussian_unit_rows(2, 600, dims)
    corpus[40000:40600] = centre[None, :] + np.float32(0.05) * noise
    corpus[5] = 0.0
    corpus[7, 3] = np.nan
    corpus[11, 0] = np.inf
    corpus[13, 1] = -np.inf
    corpus[15] = corpus[14]
    eng = make_engine(wax, 0, dims, corpus)
    queries = oracle.gaussian_unit_queries(64, dims, seed=3)
    queries[:32] = centre[None, :] + np.float32(0.02) * oracle.gaussian_unit_rows(4, 32, dims)
    queries[40] = 0.0
    queries[41] = corpus[14]
    for survivors, div in [(8, 64), (2, 64), (64, 64), (8, 4), (8, 4096)]:
        eng.setTuning("batch_survivors", survivors)
        eng.setTuning("batch_sample_div", div)
        before1 = eng.getTuning("onepass_queries")
        _batch_vs_single(eng, queries, 30)
        assert eng.getTuning("onepass_queries") - before1 == 64, (survivors, div)
    eng.close()


def test_search_batch_hits_device_resident(wax):
    """wax_hip_search_batch_hits_device: queries and hits stay in HBM; equals the host-pointer call bit for bit — through
    the one-pass pipeline, the slab pipeline, the loop path (small batch / unsupported dims), with wider and narrower
    row strides, more than 1024 queries, and an empty engine."""
    import torch
    from wax_amd import sharded
    dev = torch.device("cuda", 0)
    KEY_PAD = (1 << 63) - 1

    def run(eng, queries, k, stride):
        dq = torch.from_numpy(np.ascontiguousarray(queries)).to(dev)
        out = torch.full((len(queries), stride, 2), 5, dtype=torch.int64, device=dev)
        guard = torch.full((8,), 77, dtype=torch.int64, device=dev)
        eng.searchBatchHitsDevice(dq.data_ptr(), len(queries), k, out.data_ptr(), stride, torch.cuda.current_stream(dev).cuda_stream)
        assert torch.all(guard == 77)
        return out.cpu().numpy()

    for dims, n, nq in [(384, 80_000, 300), (384, 20_000, 300), (100, 5_000, 20), (384, 80_000, 3), (384, 70_000, 1500)]:
        corpus = oracle.gaussian_unit_rows(21, n, dims)
        eng = make_engine(wax, 0, dims, corpus, np.arange(n, dtype=np.uint64) + 1000)
        queries = oracle.gaussian_unit_queries(nq, dims, seed=n % 97)
        for k, stride in [(10, 10), (10, 16), (10, 4)]:
            hits = run(eng, queries, k, stride)
            ref, _ = eng.searchBatchHits(queries, k)
            w = min(k, stride)
            assert np.array_equal(hits[:, :w], ref[:, :w]), (dims, n, nq, k, stride)
            assert np.all(hits[:, w:, 0] == KEY_PAD) and np.all(hits[:, w:, 1] == -1)
        d_ids, d_scores, valid = sharded.sharded_search_batch(eng, queries[:min(64, nq)], 10, world=1)       # device-resident exchange path
        for i in (0, min(63, nq - 1)):
            s_ids, s_scores = eng.searchArrays(queries[i], 10)
            assert np.array_equal(d_ids[i][valid[i]], s_ids) and np.array_equal(d_scores[i][valid[i]], s_scores)
        eng.close()
    empty = wax.HIPVectorEngine(dimensions=64)
    hits = run(empty, oracle.gaussian_unit_queries(5, 64), 10, 10)
    assert np.all(hits[:, :, 0] == KEY_PAD)
    with pytest.raises(wax.EncodingError):
        empty.searchBatchHitsDevice(0, 4, 10, 0, 10)


@pytest.mark.parametrize("dims,n", [(384, 4_096), (384, 9_000), (384, 33_333), (768, 2_100), (768, 20_000), (128, 60_000)])
def test_small_stores_take_the_one_pass_pipeline(wax, dims, n):
    """Since round 6 the one-pass MFMA pipeline (sample -> thresholds -> filtering GEMM -> finish) answers stores from 64 units of 64
    rows (32 at D = 768) up instead of from 65 536 rows ("batch_onepass_tiles", default 64): top_k 10 / 100 / 300 and a ragged batch
    equal the single-query answers bit for bit, the one-pass counter says which pipeline ran, and the old floor (slab pipeline, or one
    scan per query beyond its top_k limit) gives the same hits."""
    corpus = oracle.gaussian_unit_rows(n % 89, n, dims)
    eng = make_engine(wax, 0, dims, corpus, np.arange(n, dtype=np.uint64) * 7 + 2)
    assert eng.getTuning("batch_onepass_tiles") == 64
    queries = oracle.gaussian_unit_queries(77, dims, seed=n % 31)
    for k in (10, 100, 300):
        o0 = eng.getTuning("onepass_queries")
        hits, counts = eng.searchBatchHits(queries, k)
        took = eng.getTuning("onepass_queries") - o0       # (a top_k that needs a quarter of a tiny store as candidates is not planned)
        assert took == len(queries) or (k > 10 and took == 0 and n < 30_000), (dims, n, k, took)
        for i in (0, 5, 38, 76):
            s_ids, s_scores = eng.searchArrays(queries[i], k)
            b_ids, b_scores = wax.HIPVectorEngine.hitsToResults(wax.VectorMetric.cosine, hits[i, :counts[i]])
            assert np.array_equal(b_ids, s_ids) and np.array_equal(b_scores, s_scores), (dims, n, k, i)
        eng.setTuning("batch_onepass_tiles", 1024)
        o0 = eng.getTuning("onepass_queries")
        old_hits, old_counts = eng.searchBatchHits(queries, k)
        assert eng.getTuning("onepass_queries") == o0
        assert np.array_equal(old_hits, hits) and np.array_equal(old_counts, counts), (dims, n, k)
        eng.setTuning("batch_onepass_tiles", 64)
    with pytest.raises(wax.WaxError):
        eng.setTuning("batch_onepass_tiles", 31)
    eng.close()


def test_host_pointer_batches_outside_the_mfma_pipelines_share_exact_passes(wax):
    """A host-pointer batch of at least 16 queries that no MFMA pipeline takes (top_k 100 on a store below the one-pass floor;
    "batch_mode" 0) is answered by shared exact passes — 16 queries per pass over the f32 store, the single-query kernel's arithmetic —
    instead of one scan per query ("batch_host_multi", default 1): the single-query hits bit for bit, the pass counter moves, and
    the per-query loop ("batch_host_multi" 0) returns the same."""
    dims, n = 384, 3_000
    corpus = oracle.gaussian_unit_rows(5, n, dims)
    eng = make_engine(wax, 0, dims, corpus, np.arange(n, dtype=np.uint64) * 3 + 9)
    queries = oracle.gaussian_unit_queries(41, dims, seed=19)
    assert eng.getTuning("batch_host_multi") == 1
    for mode, k in ((1, 100), (1, 192), (0, 10), (0, 100)):                  # (batch_mode, top_k)
        eng.setTuning("batch_mode", mode)
        p0, b0 = eng.getTuning("batch_multi_passes"), eng.getTuning("batch_queries")
        hits, counts = eng.searchBatchHits(queries, k)
        assert eng.getTuning("batch_multi_passes") - p0 == 3 and eng.getTuning("batch_queries") == b0, (mode, k)   # 41 queries = 3 passes
        for i in (0, 15, 16, 40):
            s_ids, s_scores = eng.searchArrays(queries[i], k)
            b_ids, b_scores = wax.HIPVectorEngine.hitsToResults(wax.VectorMetric.cosine, hits[i, :counts[i]])
            assert np.array_equal(b_ids, s_ids) and np.array_equal(b_scores, s_scores), (mode, k, i)
        eng.setTuning("batch_host_multi", 0)
        p0 = eng.getTuning("batch_multi_passes")
        loop_hits, loop_counts = eng.searchBatchHits(queries, k)
        assert eng.getTuning("batch_multi_passes") == p0
        assert np.array_equal(loop_hits, hits) and np.array_equal(loop_counts, counts), (mode, k)
        eng.setTuning("batch_host_multi", 1)
    eng.close()


def test_device_resident_batch_waits_for_a_busy_caller_stream_only(wax):
    """The library's stream is ordered behind the caller's `stream` while that stream still has work pending — here milliseconds
    of matrix products in front of the copy that produces the queries — and skips the event when the stream has drained
    ("batch_in_wait" 0, the default; 1 = always record + wait). Both settings, busy and idle stream: the host-pointer call's hits."""
    import torch
    dev = torch.device("cuda", 0)
    dims, n, nq, k = 384, 120_000, 256, 10
    corpus = oracle.gaussian_unit_rows(77, n, dims)
    eng = make_engine(wax, 0, dims, corpus, np.arange(n, dtype=np.uint64) + 5)
    queries = oracle.gaussian_unit_queries(nq, dims, seed=41)
    ref, _ = eng.searchBatchHits(queries, k)
    good = torch.from_numpy(np.ascontiguousarray(queries)).to(dev)
    a = torch.randn((4096, 4096), device=dev)
    torch.cuda.synchronize()
    st = torch.cuda.current_stream(dev)
    assert eng.getTuning("batch_in_wait") == 0
    for mode in (0, 1, 0):
        eng.setTuning("batch_in_wait", mode)
        for busy in (True, False, True):
            dq = torch.full((nq, dims), float("nan"), device=dev)
            out = torch.zeros((nq, k, 2), dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            if busy:
                b = a
                for _ in range(12):
                    b = torch.mm(b, a) * 1e-3                      # a few milliseconds on the caller's stream ...
                dq.copy_(good, non_blocking=True)                # ... in front of the copy that produces the queries
                assert not st.query()                            # still pending when the library is called
            else:
                dq.copy_(good)
                torch.cuda.synchronize()
            eng.searchBatchHitsDevice(dq.data_ptr(), nq, k, out.data_ptr(), k, st.cuda_stream)
            assert np.array_equal(out.cpu().numpy(), ref), (mode, busy)
    eng.close()


def test_concurrent_batched_searches_share_the_mirror(wax):
    """Batched searches are re-entrant like every other read entry point: four threads batch-search at once (pooled
    per-call workspaces, one shared bf16 mirror), interleaved with single-query searches and a writer."""
    dims, n = 384, 80_000
    corpus = oracle.gaussian_unit_rows(31, n, dims)
    eng = make_engine(wax, 0, dims, corpus)
    queries = oracle.gaussian_unit_queries(128, dims, seed=12)
    ref = eng.searchBatch(queries, 10)
    errors = []

    def worker(tid):
        try:
            for it in range(6):
                ids, scores, counts = eng.searchBatch(queries, 10)
                assert np.array_equal(ids, ref[0]) and np.array_equal(scores, ref[1])
                s_ids, _ = eng.searchArrays(queries[tid], 10)
                assert np.array_equal(s_ids, ref[0][tid])
        except Exception as ex:  # noqa: BLE001
            errors.append((tid, ex))

    ts = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    # a mutation in between invalidates the mirror for everyone
    eng.add(10 ** 9, queries[5])
    ids, scores, _ = eng.searchBatch(queries, 10)
    assert ids[5, 0] == 10 ** 9 and abs(scores[5, 0] - 1.0) <= 1e-5
    eng.close()


@pytest.mark.parametrize("metric", [0, 1, 2])
@pytest.mark.parametrize("dims", [64, 128, 256, 384, 512, 768, 1024, 1536])
def test_multi_query_exact_scan_is_bit_identical(wax, dims, metric):
    """scan_multi_kernel (the shared exact pass of the batched path's fallback, multiscan.hip) against scan_kernel:
    with the MFMA pipelines switched off, a device-resident batch is answered by groups of queries sharing one pass
    over the f32 store — the hits (keys = ordered distance : row, frame ids) must equal the single-query path's BIT FOR
    BIT, at every specialised dimension and metric, for k below and above the 64-slot list limit, for group remainders,
    ragged row counts, a non-zero row base, and against `batch_multi = 0` (one scan per query, the round-2 fallback)."""
    import torch
    dev = torch.device("cuda", 0)
    n = 30_011 if dims <= 512 else 9_973
    corpus = oracle.gaussian_unit_rows(40 + dims, n, dims)
    if metric != 0:
        corpus = corpus * np.linspace(0.5, 2.0, n, dtype=np.float32)[:, None]
    corpus[17] = corpus[16]                                   # an exact tie: (distance asc, row asc) must decide
    eng = make_engine(wax, metric, dims, corpus, np.arange(n, dtype=np.uint64) * 5 + 3)
    eng.setRowBase(1_000_003)
    eng.setTuning("batch_mode", 0)                            # no MFMA pipeline: the exact path answers the batch
    group, group_big = eng.getTuning("batch_multi_group"), eng.getTuning("batch_multi_group_big")   # queries per pass: k <= 60 / k <= 192
    assert group == 16 and group_big in (0, 16)               # 0: the 256-slot lists of 16 queries do not fit beside the query block (dims >= 512)
    for nq, k in [(group * 2 + 3, 10), (1, 10), (2, 60), (group_big + 1, 100), (5, 192), (17, 30)]:
        queries = oracle.gaussian_unit_queries(nq, dims, seed=dims + nq + k)
        if nq > 2:
            queries[2] = corpus[16]                           # aims at the tie
        dq = torch.from_numpy(np.ascontiguousarray(queries)).to(dev)
        out = {}
        for multi in (1, 0):
            eng.setTuning("batch_multi", multi)
            p0 = eng.getTuning("batch_multi_passes")
            o = torch.full((nq, k + 2, 2), 5, dtype=torch.int64, device=dev)
            eng.searchBatchHitsDevice(dq.data_ptr(), nq, k, o.data_ptr(), k + 2, torch.cuda.current_stream(dev).cuda_stream)
            out[multi] = o.cpu().numpy()
            passes = eng.getTuning("batch_multi_passes") - p0
            g_k = group if k <= 60 else group_big
            assert passes == ((-(-nq // g_k)) if (multi and nq >= 2 and g_k >= 2) else 0), (dims, metric, nq, k, multi, passes)
        assert np.array_equal(out[1], out[0]), (dims, metric, nq, k)
        for i in range(nq):                                   # and both equal the single-query entry point
            s_ids, s_scores = eng.searchArrays(queries[i], k)
            hits = out[1][i]
            assert np.array_equal(hits[:len(s_ids), 1].astype(np.uint64), s_ids), (dims, metric, nq, k, i)
            assert np.all(hits[k:, 0] == (1 << 63) - 1)
    eng.close()


def _merges_in_kernel(grid, k, n, dims):
    """kernels.h scan_merges_in_kernel: any k <= 192 on grids <= 160 (wave-list merge); k <= 64 on every default grid (<= 512:
    the k-way merge of the lists' heads) for stores of up to 2 GiB of rows."""
    return grid <= 160 or (k <= 64 and grid <= 512 and n * dims * 4 <= 2 << 30)


def test_fused_final_merge_equals_two_launch_path(wax):
    """Small grids (<= 160 workgroups: stores up to ~20K rows) let the scan kernel's last-arriving workgroup do the final
    merge (scan_epilogue: write-through partial lists, device-scope ticket) instead of a second launch. Same hits, bit for
    bit, as the two-launch path ("fuse_merge" = 0) — for every k the fused kernels serve, ragged sizes, all metrics, the
    generic-dims kernel, and many back-to-back queries on pipelined slots (the ticket must re-arm itself). For k <= 64 the last
    arriver merges the lists' heads (kway_merge: one or two lists per thread), which serves every default grid (<= 512), so
    larger stores take the same path; there k > 64 stays on two launches and both settings run the same kernels."""
    for metric, dims, n in [(0, 384, 10_000), (1, 384, 9_999), (2, 128, 5_000), (0, 768, 3_001), (0, 100, 2_000), (0, 384, 65), (0, 64, 20_000),
                            (0, 384, 45_001), (2, 768, 70_000), (1, 384, 400_000), (0, 100, 150_000)]:   # grids of 257 .. 512: two lists per thread (k <= 64)
        corpus = oracle.gaussian_unit_rows(7 + n, n, dims)
        corpus[11] = corpus[10]
        eng = make_engine(wax, metric, dims, corpus, np.arange(n, dtype=np.uint64) + 9)
        queries = oracle.gaussian_unit_queries(24, dims, seed=n)
        queries[3] = corpus[10]
        for k in (1, 3, 4, 5, 10, 24, 32, 33, 47, 64, 65, 192):
            eng.setTuning("fuse_merge", 1)
            pend = [eng.submit(q, k) for q in queries[:4]]          # pipelined: four slots, four tickets
            fused = [eng.collect(t, k) for t in pend] + [eng.searchArrays(q, k) for q in queries[4:]]
            if k <= 64:                                             # k <= 64 merges the lists' heads ("merge_kway"); the wave-list merge must agree
                eng.setTuning("merge_kway", 0)
                for q, (f_ids, f_scores) in zip(queries[:8], fused):
                    w_ids, w_scores = eng.searchArrays(q, k)
                    assert np.array_equal(f_ids, w_ids) and np.array_equal(f_scores, w_scores), ("kway", metric, dims, n, k)
                eng.setTuning("merge_kway", 1)
            eng.setTuning("fuse_merge", 0)
            for q, (f_ids, f_scores) in zip(queries, fused):
                s_ids, s_scores = eng.searchArrays(q, k)
                assert np.array_equal(f_ids, s_ids) and np.array_equal(f_scores, s_scores), (metric, dims, n, k)
        e_ids, e_scores, _, _ = oracle.search(metric, corpus, np.arange(n, dtype=np.uint64) + 9, queries[0], 10)
        eng.setTuning("fuse_merge", 1)
        g_ids, g_scores = eng.searchArrays(queries[0], 10)
        assert_parity(g_ids, g_scores, e_ids, e_scores, None, f"fused merge m{metric} d{dims} n{n}")
        eng.close()


def test_fused_merge_hand_over_litmus_under_l2_pressure(wax):
    """Litmus for the fused final merge's hand-over (kernels.hip::scan_epilogue): every workgroup publishes its k keys with
    relaxed agent-scope (write-through) stores, drains them (`s_waitcnt vmcnt(0)`), takes a relaxed agent-scope ticket; the last
    arriver reads the other lists with agent-scope loads. That is an argument about what gfx950 does with sc1 stores and L2-resident
    atomics, not a release / acquire pair the language guarantees — so this test hammers it where a violation would show: hundreds of
    thousands of one-launch scans on grids of 157 / 417 / 469 workgroups (one and two lists per thread of the k-way merge, the
    wave-list merge at k = 100), from four host threads with four tickets each in flight (slots and tickets re-armed back to back), while a co-running
    copy kernel streams 1 GB through every XCD's L2 and HBM channel. Every answer is compared, id for id and score for score,
    with the two-launch path's ("fuse_merge" = 0: partial lists cross a kernel boundary). A stale partial list would surface as a
    missing or duplicated neighbour in some top-k; a lost ticket as a collect that never returns (the per-test timeout)."""
    import threading
    import time
    import torch
    dev = torch.device("cuda", 0)
    dims = 384
    stores = []
    for n in (10_000, 40_000, 120_000):                       # 157 workgroups (two chunks per wave; one list per thread), 417 and 469 (two lists per thread)
        corpus = oracle.gaussian_unit_rows(31 + n, n, dims)
        eng = make_engine(wax, 0, dims, corpus, np.arange(n, dtype=np.uint64) + 5)
        eng.setTuning("slots", 16)
        eng.setTuning("streams", 4)
        queries = oracle.gaussian_unit_queries(48, dims, seed=n)
        ref = {}
        eng.setTuning("fuse_merge", 0)
        for k in (10, 30, 100):
            ref[k] = [eng.searchArrays(q, k) for q in queries]
        eng.setTuning("fuse_merge", 1)
        assert (eng.getTuning("scan_grid") <= 160) == (n == 10_000) and eng.getTuning("scan_grid") <= 512, eng.getTuning("scan_grid")
        stores.append((eng, queries, ref))
    stop = threading.Event()
    side = torch.cuda.Stream(device=dev)
    a = torch.empty(256 << 20, dtype=torch.uint8, device=dev)
    b = torch.empty(256 << 20, dtype=torch.uint8, device=dev)

    def thrash():                                             # 2 x 256 MB per copy pair: no line of any L2 survives it
        with torch.cuda.stream(side):
            while not stop.is_set():
                for _ in range(8):
                    b.copy_(a, non_blocking=True)
                    a.copy_(b, non_blocking=True)
                side.synchronize()
    errors, done = [], [0] * 4

    def worker(w, deadline):
        rng = np.random.default_rng(1000 + w)
        try:
            while time.perf_counter() < deadline and not errors:
                eng, queries, ref = stores[int(rng.integers(len(stores)))]
                k = int(rng.choice([10, 10, 30, 100]))
                order = rng.integers(len(queries), size=64)
                pend = []
                for qi in order:
                    if len(pend) == 4:
                        t, j = pend.pop(0)
                        ids, scores = eng.collect(t, k)
                        if not (np.array_equal(ids, ref[k][j][0]) and np.array_equal(scores, ref[k][j][1])):
                            errors.append((w, k, int(j), ids[:5].tolist(), ref[k][j][0][:5].tolist()))
                            return
                        done[w] += 1
                    pend.append((eng.submit(queries[qi], k), qi))
                for t, j in pend:
                    ids, scores = eng.collect(t, k)
                    if not (np.array_equal(ids, ref[k][j][0]) and np.array_equal(scores, ref[k][j][1])):
                        errors.append((w, k, int(j), ids[:5].tolist(), ref[k][j][0][:5].tolist()))
                        return
                    done[w] += 1
        except Exception as ex:  # noqa: BLE001
            errors.append((w, repr(ex)))
    th = threading.Thread(target=thrash)
    th.start()
    deadline = time.perf_counter() + 12.0
    ws = [threading.Thread(target=worker, args=(w, deadline)) for w in range(4)]
    [t.start() for t in ws]
    [t.join() for t in ws]
    stop.set()
    th.join()
    torch.cuda.synchronize()
    merged = sum(int(e.getTuning("merged_scans")) for e, _, _ in stores)
    print(f"\n[litmus] {sum(done)} one-launch scans checked against the two-launch path under L2 / HBM pressure ({merged} merged in their own kernel)")
    assert not errors, errors[:2]
    assert sum(done) >= 20_000 and merged >= sum(done) // 2     # (k = 100 on the two larger grids takes two launches: same comparison, different path)
    for e, _, _ in stores:
        e.close()


def test_query_in_kernel_arguments_equals_uploaded_query(wax):
    """"query_args": a single-query scan may take its query through the kernel arguments (scan_kernel_qarg: the dims floats ride
    in the launch packet, no upload copy on the stream). Same kernel body, so the hits must be bit-identical to the uploaded-query
    path — for both dimensions that have the kernel (384, 768), all metrics, both selection capacities (k <= 64, k <= 192),
    ragged sizes, pipelined tickets, the two-launch merge, and on a sharded handle. Mode 1 (default) uses it only where the
    scan grid is small (launch-latency-bound stores), mode 2 everywhere; k > 192 (general selection) and other dimensions never do."""
    for metric, dims, n in [(0, 384, 10_000), (1, 384, 9_999), (2, 768, 3_001), (0, 768, 150_000), (0, 384, 400_000)]:
        corpus = oracle.gaussian_unit_rows(17 + n, n, dims)
        corpus[11] = corpus[10]
        eng = make_engine(wax, metric, dims, corpus, np.arange(n, dtype=np.uint64) + 9)
        queries = oracle.gaussian_unit_queries(12, dims, seed=n)
        queries[3] = corpus[10]
        grid = eng.getTuning("scan_grid")
        eng.setTuning("merge_overlap_mb", 0)        # (pipelined scans over >= 400 MB would otherwise take the two-launch form: its own test)
        for k in (1, 10, 64, 65, 192, 500):
            small = _merges_in_kernel(grid, k, n, dims)                 # mode 1: where the scan is the query's only packet
            eng.setTuning("query_args", 0)
            ref = [eng.searchArrays(q, k) for q in queries]
            for mode in (1, 2):
                eng.setTuning("query_args", mode)
                before = eng.getTuning("query_args_scans")
                pend = [eng.submit(q, k) for q in queries[:4]]
                got = [eng.collect(t, k) for t in pend] + [eng.searchArrays(q, k) for q in queries[4:]]
                used = eng.getTuning("query_args_scans") - before
                assert used == (len(queries) if (k <= 192 and (mode == 2 or small)) else 0), (metric, dims, n, k, mode, used)
                for (a_ids, a_scores), (b_ids, b_scores) in zip(ref, got):
                    assert np.array_equal(a_ids, b_ids) and np.array_equal(a_scores, b_scores), (metric, dims, n, k, mode)
        eng.setTuning("query_args", 2)
        eng.setTuning("fuse_merge", 0)                                  # two launches: scan (query in its arguments) + merge
        a = eng.searchArrays(queries[0], 10)
        eng.setTuning("query_args", 0)
        b = eng.searchArrays(queries[0], 10)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (metric, dims, n)
        eng.close()
    # other dimensions: never (no kernel), and nothing breaks
    eng = make_engine(wax, 0, 128, oracle.gaussian_unit_rows(1, 5000, 128))
    eng.setTuning("query_args", 2)
    eng.searchArrays(oracle.gaussian_unit_queries(1, 128)[0], 10)
    assert eng.getTuning("query_args_scans") == 0
    eng.close()
    # sharded handle: every shard's scan takes the query in its arguments; same answers as one engine
    n, dims = 30_000, 384
    corpus = oracle.gaussian_unit_rows(5, n, dims)
    one = make_engine(wax, 0, dims, corpus)
    many = wax.HIPVectorEngine(dimensions=dims, devices=[0, 0, 0])
    many.setTuning("shard_min_mb", 0)                          # spread these 46 MB over the three shards (the default keeps them on one)
    many.addBatch(np.arange(n, dtype=np.uint64), corpus)
    for q in oracle.gaussian_unit_queries(6, dims, seed=8):
        a, b = one.searchArrays(q, 10), many.searchArrays(q, 10)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert many.getTuning("query_args_scans") == 18
    one.close(), many.close()


def test_device_side_full_retry_equals_host_retry_and_exact_path(wax):
    """Dense neighbourhoods: more rows inside the bf16 error band of the k-th neighbour than the k' candidates of the first finish
    cover, so its certificate fails with nothing dropped. Round 4: while recent batches had such queries ("retry_hint"), a
    device-side kernel rides behind the finish kernel and re-scores ALL survivors of every uncertified query — no host round trip.
    The three ladders ("batch_retry" 1 device + host, 2 host only, 0 exact path only) must give the single-query answers bit for
    bit; the first batch arms the hint (its failures are settled from the host), later batches are settled on the device."""
    import torch
    dev = torch.device("cuda", 0)
    n, dims, nq = 300_000, 384, 256
    g = torch.Generator(device=dev).manual_seed(11)
    centres = torch.randn((20, dims), device=dev, generator=g)
    which = torch.randint(0, 20, (n,), device=dev, generator=g)
    rows = torch.nn.functional.normalize(centres[which] + 0.3 * torch.randn((n, dims), device=dev, generator=g), dim=1).contiguous()
    rows[5000:5040] = rows[4999]                                     # plus a 40-fold exact tie
    eng = wax.HIPVectorEngine(dimensions=dims)
    eng.addBatchDevice(np.arange(n, dtype=np.uint64) + 3, rows)
    q = torch.randn((nq, dims), device=dev, generator=g)
    q[: nq // 2] = rows[:nq // 2] + 0.05 * q[: nq // 2]              # half of the queries inside a cluster
    q[7] = rows[4999]
    queries = q.cpu().numpy()
    for k in (10, 100):
        ref = None
        # (the last entry re-scores EVERY survivor on the device, "batch_debug" bit 16, instead of only those the first finish's
        # exact k-th cannot exclude: same answers, same certificates)
        for mode, hint, dbg in ((1, 0, 0), (1, None, 0), (2, 0, 0), (0, 0, 0), (1, 16, 0), (1, 16, 65536)):
            eng.setTuning("batch_retry", mode)
            eng.setTuning("batch_debug", dbg)
            if hint is not None:
                eng.setTuning("retry_hint", hint)
            h0 = eng.getTuning("retry_hint")
            i0, r0, f0 = eng.getTuning("batch_inline_retries"), eng.getTuning("batch_retries"), eng.getTuning("batch_fallbacks")
            got = eng.searchBatch(queries, k)
            inl, ret, fb = eng.getTuning("batch_inline_retries") - i0, eng.getTuning("batch_retries") - r0, eng.getTuning("batch_fallbacks") - f0
            print(f"\n[device retry] k {k} batch_retry {mode} hint {h0} debug {dbg}: on the device {inl}, retries {ret}, exact-path fallbacks {fb}")
            if mode != 1 or h0 == 0:
                assert inl == 0, (k, mode, h0, inl)                   # the kernel is not even launched
            if mode == 0:
                assert ret == 0
            if k == 100:
                assert ret + fb >= 20, (mode, ret, fb)                # the dense neighbourhoods really defeat the first finish
                if mode == 1 and h0 > 0:
                    assert inl >= 20 and inl == ret, (inl, ret)       # ... and the device rung takes the whole load
                if mode == 1 and hint == 0:
                    assert eng.getTuning("retry_hint") == 16          # armed by this batch's failures
            if ref is None:
                ref = got
                for i in (0, 7, 100, 200, 255):
                    s_ids, s_scores = eng.searchArrays(queries[i], k)
                    assert np.array_equal(got[0][i, :len(s_ids)], s_ids) and np.array_equal(got[1][i, :len(s_ids)], s_scores), (k, i)
            else:
                assert all(np.array_equal(x, y) for x, y in zip(got, ref)), (k, mode, hint, dbg)
        eng.setTuning("batch_debug", 0)
        # k = 100: k' is capped at 192 (fused finish kernel) because the device retry stands behind it; k' = 2k + 32 = 232 (the
        # three-launch finish) must give the same answers
        eng.setTuning("batch_kp_fused", 0)
        got = eng.searchBatch(queries, k)
        assert all(np.array_equal(x, y) for x, y in zip(got, ref)), (k, "batch_kp_fused 0")
        eng.setTuning("batch_kp_fused", 1)
    eng.close()


def test_completion_word_equals_event_completion(wax):
    """"done_flag" (default 1): a single-query scan that merges in the kernel publishes a completion word in pinned memory behind its
    hits and collect polls that word instead of an event recorded behind the kernel. Same hits as with events ("done_flag" = 0),
    pipelined tickets collected in any order, slots reused thousands of times (the word is a per-slot sequence number), mixed
    with scans that cannot use it (two-launch merge, general selection, timed kernels)."""
    for metric, dims, n in [(0, 384, 10_000), (1, 768, 2_000), (2, 128, 5_000), (0, 100, 3_000), (0, 384, 120_000)]:
        corpus = oracle.gaussian_unit_rows(3 + n, n, dims)
        eng = make_engine(wax, metric, dims, corpus, np.arange(n, dtype=np.uint64) + 5)
        queries = oracle.gaussian_unit_queries(16, dims, seed=n)
        grid = eng.getTuning("scan_grid")
        eng.setTuning("done_flag", 0)
        ref = {k: [eng.searchArrays(q, k) for q in queries] for k in (1, 10, 100, 500)}
        eng.setTuning("done_flag", 1)
        w0 = eng.getTuning("done_flag_waits")
        for k in (1, 10, 100, 500):
            pend = [(i, eng.submit(queries[i], k)) for i in range(4)]
            got = {}
            for i, t in reversed(pend):                                 # collected in reverse order
                got[i] = eng.collect(t, k)
            for i in range(4, 16):
                got[i] = eng.searchArrays(queries[i], k)
            for i in range(16):
                assert np.array_equal(got[i][0], ref[k][i][0]) and np.array_equal(got[i][1], ref[k][i][1]), (metric, dims, n, k, i)
        used = eng.getTuning("done_flag_waits") - w0
        assert used == 16 * sum(_merges_in_kernel(grid, k, n, dims) for k in (1, 10, 100)), (metric, dims, n, used)   # k = 500 is the general selection
        for _ in range(2000):                                           # the per-slot sequence numbers keep counting
            eng.searchArrays(queries[0], 10)
        a = eng.searchArrays(queries[1], 10)
        assert np.array_equal(a[0], ref[10][1][0])
        eng.setTuning("time_kernels", 1)                                # timed kernels complete through their events
        w1 = eng.getTuning("done_flag_waits")
        b = eng.searchArrays(queries[2], 10)
        assert eng.getTuning("done_flag_waits") == w1 and np.array_equal(b[0], ref[10][2][0])
        eng.setTuning("time_kernels", 0)
        eng.setTuning("fuse_merge", 0)                                  # two launches: the merge kernel does not publish the word
        c = eng.searchArrays(queries[3], 10)
        assert eng.getTuning("done_flag_waits") == w1 and np.array_equal(c[0], ref[10][3][0])
        eng.close()


def test_certificate_bound_survives_aligned_rounding_errors(wax):
    """bf16 keeps 8 significant bits: rounding moves an element by up to 2^-8 of itself, so a dot product of two rounded unit
    vectors can be off by 2^-7 when the errors line up — twice the constant rounds 1-3 took for the worst case. The construction:
    row A = a unit vector whose every element loses 2^-8 to rounding (helpers.bf16_adversarial_unit_vector); the query is A
    itself, so its approximate similarity to A is 0.9923 instead of 1. Around it sit 300 rows at exact cosine distance
    0.0030 - 0.0065 whose approximate distances are honest: they fill the k' candidates, A is NOT among them, and with the old
    bound the certificate `a_max - eps > exact k-th` passed (0.0065 - 0.0039 > 0.0025) and the batch returned a neighbour instead
    of A. The measured bound (||q~ - q|| + max ||v~ - v|| ~ 0.0077 here) refuses, the ladder answers exactly."""
    from helpers import bf16_adversarial_unit_vector
    dims, n = 384, 40_000
    rng = np.random.default_rng(8)
    corpus = oracle.gaussian_unit_rows(77, n, dims)
    a = bf16_adversarial_unit_vector(dims)
    corpus[1234] = a
    # neighbours of A at controlled exact distances: normalise(A + t * u), u orthogonal to A, cos = 1 / sqrt(1 + t^2)
    for j, dist in enumerate(np.linspace(0.0030, 0.0065, 300)):
        u = rng.standard_normal(dims)
        u -= (u @ a.astype(np.float64)) * a.astype(np.float64)
        u /= np.linalg.norm(u)
        t = np.sqrt(1.0 / (1.0 - dist) ** 2 - 1.0)
        v = a.astype(np.float64) + t * u
        corpus[2000 + j] = (v / np.linalg.norm(v)).astype(np.float32)
    eng = make_engine(wax, 0, dims, corpus, np.arange(n, dtype=np.uint64) + 1)
    queries = oracle.gaussian_unit_queries(32, dims, seed=9)
    queries[3] = a
    queries[17] = a
    for onepass in (0, 1):
        eng.setTuning("batch_onepass", onepass)
        eng.setTuning("batch_onepass_tiles", 64 if onepass else 1024)      # (40 000 rows: the one-pass pipeline really runs)
        for k in (1, 5):
            ids, scores, counts = eng.searchBatch(queries, k)
            for i in range(len(queries)):
                s_ids, s_scores = eng.searchArrays(queries[i], k)
                assert np.array_equal(ids[i, :counts[i]], s_ids) and np.array_equal(scores[i, :counts[i]], s_scores), (onepass, k, i)
            assert ids[3, 0] == 1235 and ids[17, 0] == 1235 and abs(scores[3, 0] - 1.0) < 1e-6   # A itself, not a neighbour
    # the measured quantities: this store's worst row loses ~0.0038 to rounding (a Gaussian unit row ~0.0018)
    assert 3.5e6 < eng.getTuning("batch_max_row_err_e9") < 4.0e6
    eng.close()



def test_kernel_bound_timing_equals_bracketed_answers_and_is_not_longer(wax):
    """"time_kernels" = 2 binds the HIP event pair to the kernel's dispatch (hipExtLaunchKernel) instead of recording it in front of
    and behind the launch ("time_kernels" = 1). Same hits under both (single-query scans that merge in the kernel, the two-launch
    merge, the general selection, a batch through the filtering GEMM); every timed launch is counted; the kernel-bound mean is the
    bracketed one minus the packets around the kernel — positive, never longer (bench.kernel_bound_plausible is the rule bench.py
    applies before it prices the roofline with it)."""
    import bench
    dims, n = 384, 200_000
    corpus = oracle.gaussian_unit_rows(11, n, dims)
    eng = make_engine(wax, 0, dims, corpus, np.arange(n, dtype=np.uint64) + 3)
    queries = oracle.gaussian_unit_queries(24, dims, seed=5)
    ref = {k: [eng.searchArrays(q, k) for q in queries] for k in (10, 100, 500)}
    eng.setTuning("streams", 2)
    eng.setTuning("slots", 4)
    means = {}
    for mode in (1, 2):
        eng.setTuning("time_kernels", mode)
        for k in (10, 100, 500):
            pend = [eng.submit(q, k) for q in queries[:4]]
            got = [eng.collect(t, k) for t in pend] + [eng.searchArrays(q, k) for q in queries[4:]]
            for i in range(len(queries)):
                assert np.array_equal(got[i][0], ref[k][i][0]) and np.array_equal(got[i][1], ref[k][i][1]), (mode, k, i)
        eng.setTuning("fuse_merge", 0)
        c = eng.searchArrays(queries[0], 10)
        assert np.array_equal(c[0], ref[10][0][0])
        eng.setTuning("fuse_merge", 1)
        eng.setTuning("reset_stats", 1)
        for _ in range(3):
            for q in queries:
                eng.searchArrays(q, 10)
        st = eng.stats()
        assert int(st.scan_kernels_timed) == 3 * len(queries), (mode, st.scan_kernels_timed)
        means[mode] = st.scan_kernel_ms_total / st.scan_kernels_timed
    assert bench.kernel_bound_plausible(means[2], means[1]), means
    # the filtering GEMM of a batch
    bq = oracle.gaussian_unit_queries(64, dims, seed=6)
    eng.setTuning("time_kernels", 0)
    ids0, sc0, cn0 = eng.searchBatch(bq, 10)
    gm = {}
    for mode in (1, 2):
        eng.setTuning("time_kernels", mode)
        eng.setTuning("reset_stats", 1)
        for _ in range(4):
            ids, sc, cn = eng.searchBatch(bq, 10)
            assert np.array_equal(ids, ids0) and np.array_equal(sc, sc0) and np.array_equal(cn, cn0), mode
        st = eng.stats()
        gm[mode] = (int(st.batch_gemms_timed), st.batch_gemm_ms_total / max(1, int(st.batch_gemms_timed)))
    assert gm[1][0] == gm[2][0], gm                                  # the same launches are timed under both modes
    if gm[1][0] > 0:                                                 # (the one-pass pipeline's filtering GEMM is the timed launch)
        assert bench.kernel_bound_plausible(gm[2][1], gm[1][1]), gm
    eng.setTuning("time_kernels", 0)
    eng.close()


def test_scans_in_a_stream_of_scans_leave_the_merge_to_a_second_launch(wax):
    """"merge_overlap_mb" (default 400): a single-query scan submitted while other tickets of the engine are still out runs in a stream
    of scans, where the separate merge launch overlaps the next scan; stores of at least that size then take the two-launch form
    (uploaded query, scan, merge kernel, event), a query submitted alone keeps the single launch. Same hits either way, whatever the
    mix; the shard-device entry point applies the same rule to a ring entry whose predecessor is still running."""
    import torch
    dims, n = 384, 120_000
    corpus = oracle.gaussian_unit_rows(21, n, dims)
    eng = make_engine(wax, 0, dims, corpus, np.arange(n, dtype=np.uint64) + 9)
    queries = oracle.gaussian_unit_queries(32, dims, seed=3)
    assert eng.getTuning("merge_overlap_mb") == 400
    ref = {k: [eng.searchArrays(q, k) for q in queries] for k in (10, 64, 100)}
    assert eng.getTuning("overlap_scans") == 0                        # blocking calls: nothing else in flight
    eng.setTuning("slots", 4)
    eng.setTuning("streams", 2)

    def pipelined(k):
        got, pend = [], []
        for q in queries:
            if len(pend) == 4:
                got.append(eng.collect(pend.pop(0), k))
            pend.append(eng.submit(q, k))
        got += [eng.collect(t, k) for t in pend]
        return got

    for k in (10, 64, 100):                                           # a 184 MB store: below the default threshold, one launch each
        got = pipelined(k)
        assert all(np.array_equal(g[0], r[0]) and np.array_equal(g[1], r[1]) for g, r in zip(got, ref[k])), k
    assert eng.getTuning("overlap_scans") == 0
    eng.setTuning("merge_overlap_mb", 100)
    m0, f0 = eng.getTuning("merged_scans"), eng.getTuning("done_flag_waits")
    for k in (10, 64, 100):
        got = pipelined(k)
        assert all(np.array_equal(g[0], r[0]) and np.array_equal(g[1], r[1]) for g, r in zip(got, ref[k])), k
    # the first submit of each run found nothing in flight (one launch, completion word); the other 31 took the two-launch form
    assert eng.getTuning("overlap_scans") == 3 * 31
    # (k = 100 is beyond the k-way merge: on this grid it never merges in the kernel)
    assert eng.getTuning("merged_scans") - m0 == 2 and eng.getTuning("done_flag_waits") - f0 == 2
    a = eng.searchArrays(queries[5], 10)                              # alone again: the single launch
    assert np.array_equal(a[0], ref[10][5][0]) and eng.getTuning("overlap_scans") == 3 * 31
    # the shard-device path: 16 calls enqueued back to back on two streams against the same answers
    dev = torch.device("cuda", 0)
    streams = [torch.cuda.Stream(dev) for _ in range(2)]
    outs = [torch.empty((10, 2), dtype=torch.int64, device=dev) for _ in range(16)]
    o0 = eng.getTuning("overlap_scans")
    for i in range(16):
        eng.searchShardDevice(queries[i], 10, outs[i].data_ptr(), streams[i % 2].cuda_stream)
    torch.cuda.synchronize()
    for i in range(16):
        keys = outs[i].cpu().numpy()
        assert np.array_equal(keys[:, 1].astype(np.uint64), ref[10][i][0]), i
    assert eng.getTuning("overlap_scans") > o0                        # (how many depends on how fast the scans drain)
    eng.setTuning("merge_overlap_mb", 0)
    o1 = eng.getTuning("overlap_scans")
    got = pipelined(10)
    assert all(np.array_equal(g[0], r[0]) for g, r in zip(got, ref[10])) and eng.getTuning("overlap_scans") == o1
    eng.close()


@pytest.mark.parametrize("dims", [128, 256, 384, 512, 768])
def test_fragment_ordered_queries_equal_row_major_queries(wax, dims):
    """"batch_qfrag" (default 1): the prep kernel writes the bf16 queries a second time in MFMA A-fragment order and the
    register-resident GEMM loads its fragments from there (one contiguous 1-KB run per k-step instead of 32 rows x 32 bytes). Same
    fragments => same approximate similarities => the same thresholds, survivors, certificates and hits as with row-major reads:
    identical answers AND identical fallback / retry counters, for ragged batch sizes (padding queries) and several query groups."""
    n = 90_000
    corpus = oracle.gaussian_unit_rows(100 + dims, n, dims)
    eng = make_engine(wax, 0, dims, corpus, np.arange(n, dtype=np.uint64) + 2)
    assert eng.getTuning("batch_qfrag") == 1
    for nq in (17, 256, 300, 700):
        queries = oracle.gaussian_unit_queries(nq, dims, seed=nq + dims)
        res = {}
        for mode in (1, 0):
            eng.setTuning("batch_qfrag", mode)
            f0, r0, o0 = eng.getTuning("batch_fallbacks"), eng.getTuning("batch_retries"), eng.getTuning("onepass_queries")
            ids, scores, counts = eng.searchBatch(queries, 10)
            res[mode] = (ids, scores, counts, eng.getTuning("batch_fallbacks") - f0, eng.getTuning("batch_retries") - r0, eng.getTuning("onepass_queries") - o0)
        assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2]), (dims, nq)
        assert res[0][3:] == res[1][3:], (dims, nq, res[0][3:], res[1][3:])
        assert res[1][5] > 0, (dims, nq)                             # the one-pass pipeline (the rq kernel) answered
        for i in (0, nq // 2, nq - 1):
            s_ids, s_scores = eng.searchArrays(queries[i], 10)
            assert np.array_equal(res[1][0][i, :res[1][2][i]], s_ids) and np.array_equal(res[1][1][i, :res[1][2][i]], s_scores), (dims, nq, i)
    eng.close()
