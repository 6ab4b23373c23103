"""searchWide ("The wide finish"): the selection against its definition through the probe, the call against search(topK=k)
bit for bit and that against the f64 oracle, the certificate where its float64 restatement (mirror_wide_ref.py) holds with room."""
import numpy as np
import pytest

import mirror8_ref as R
import mirror_wide_ref as W
import oracle
from helpers import assert_parity
from wax_amd.errors import EncodingError

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def wax(hip_lib):
    import wax_amd
    if hip_lib.wax_hip_device_count() == 0:
        pytest.skip("no HIP device on this host: the gpu-marked tests run on the MI355X box (pytest -m gpu)")
    assert hip_lib.wax_hip_available() == 1, "a HIP device is visible but it is not gfx950: the HIP path needs an MI355X"
    return wax_amd


def make_engine(wax, metric, dims, corpus, ids=None, grid=0, **kw):
    eng = wax.HIPVectorEngine(metric=wax.VectorMetric(metric), dimensions=dims, **kw)
    eng.addBatch(np.arange(len(corpus), dtype=np.uint64) if ids is None else ids, corpus)
    eng.setTuning("grid_blocks", grid)
    return eng


def same(a, b):
    return np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1], equal_nan=True)


SELECT_CASES = [(n, c, fill, ties) for n in (1, 2, 3, 17, 512) for c in (1024, 4096)
                for fill in ("full", "short", "none-full", "low-tail") for ties in (False, True)]


def made_up_lists(n_lists, fill, ties, seed):
    """Unique keys. short: every other list holds fewer than 64; low-tail: list 0 lies below every other key; ties: the row word decides."""
    rng = np.random.default_rng(seed)
    live = np.full(n_lists, W.KP)
    if fill == "short":
        live[::2] = rng.integers(0, W.KP, size=len(live[::2]))
    elif fill == "none-full":
        live = rng.integers(1, W.KP, size=n_lists)
    dist = np.where(ties & (rng.random((n_lists, W.KP)) < 0.7), np.float32(0.5), rng.random((n_lists, W.KP), dtype=np.float32))
    dist[0] -= np.float32(2.0 * (fill == "low-tail"))
    keys = W.keys_of(dist, (rng.permutation(1 << 20)[:dist.size] + 7).reshape(dist.shape))
    keys[np.arange(W.KP)[None, :] >= live[:, None]] = W.PAD
    return np.sort(keys, axis=1)


def test_the_select_cases_reach_every_source():
    seen = {(c, W.select_model(made_up_lists(n, fill, ties, i), c)[2]) for i, (n, c, fill, ties) in enumerate(SELECT_CASES)}
    assert seen == {(c, s) for c in (1024, 4096) for s in (W.ALL, W.TAIL, W.RANK)}


@pytest.mark.parametrize("case", range(len(SELECT_CASES)), ids=lambda i: "-".join(map(str, SELECT_CASES[i])))
def test_select_is_its_definition(wax, case):
    n, c, fill, ties = SELECT_CASES[case]
    lists = made_up_lists(n, fill, ties, case)
    want, bound, source = W.select_model(lists, c)
    got, got_bound, got_source = wax.HIPVectorEngine.mirrorWideProbe(lists, c)
    assert (len(got), got_bound, got_source) == (len(want), bound, source) and np.array_equal(np.sort(got), want)


@pytest.mark.parametrize("n,dims,metric,grid", W.STORES)
@pytest.mark.parametrize("bits", (8, 16))
def test_search_wide_is_search_and_certifies_where_f64_does(wax, n, dims, metric, grid, bits):
    corpus = R.corpus_for(metric, n, dims)
    eng = make_engine(wax, metric, dims, corpus, grid=grid)
    held, tail_certified = 0, False
    for qi, q in enumerate(R.queries_for(dims, 2)):
        got = [eng.searchWide(q, k, bits=bits, stats=True) for k in W.KS]
        margins = W.f64_margins(corpus, metric, q, bits, W.KS, [st["candidates"] for _, _, st in got])
        for k, (ids, scores, st), margin in zip(W.KS, got, margins):
            ctx = f"{n}x{dims} metric {metric} grid {grid} bits {bits} query {qi} k {k}: {st}, f64 margin {margin}"
            exact = eng.searchArrays(q, k)
            assert same((ids, scores), exact) and st["mirror"] == bits and st["c"] == (1024 if min(k, n) <= 256 else 4096), ctx
            e_ids, e_scores, _, _ = oracle.search(metric, corpus, None, q, k)
            assert_parity(exact[0], exact[1], e_ids, e_scores, oracle.search(metric, corpus, None, q, min(k + 64, n))[1], ctx)
            assert st["certified"] + st["reran_f32"] == 1, ctx
            if margin > W.GUARD:
                held += 1
                assert st["certified"] == 1, ctx
                tail_certified |= st["bound_source"] == W.TAIL and st["candidates"] < n and k >= 257
    assert grid != 512 or held * 10 >= 9 * 2 * len(W.KS), held     # the default grid: at most one triple in ten is excused
    assert grid != 64 or tail_certified                           # ~317 rows per list: T cuts below K_C, and the answer certifies under it


@pytest.mark.parametrize("bits", (8, 16))
def test_the_certificate_fails_where_it_must_and_the_answer_stays_exact(wax, bits):
    dims, n, k = 384, 20005, 100
    q = R.queries_for(dims, 1)[0]
    # the k + 100 best rows all among the rows of workgroup 1 of 63 (16-row chunks dealt to 252 waves in turn): T sits inside the answer
    near = R.corpus_for(0, n, dims).copy()
    w = np.random.default_rng(3).standard_normal((k + 100, dims)).astype(np.float32)
    where = np.flatnonzero((np.arange(n) // 16) % 252 // 4 == 1)[:k + 100]
    near[where] = q[None, :] + 0.05 * w / np.linalg.norm(w, axis=1)[:, None] * np.linspace(0.2, 1.0, k + 100)[:, None]
    eng = make_engine(wax, 0, dims, near, grid=64)
    ids, scores, st = eng.searchWide(q, k, bits=bits, stats=True)
    assert same((ids, scores), eng.searchArrays(q, k)) and (st["certified"], st["reran_f32"], st["bound_source"], st["lists"]) == (0, 1, W.TAIL, 63), st
    flat = make_engine(wax, 0, dims, np.tile(near[5], (5000, 1)))                 # identical rows: every key ties
    ids, scores, st = flat.searchWide(q, k, bits=bits, stats=True)
    assert same((ids, scores), flat.searchArrays(q, k)) and (st["certified"], st["reran_f32"]) == (0, 1), st
    for v in (np.where(np.arange(dims) == 3, np.float32(np.nan), q), np.zeros(dims, dtype=np.float32)):    # a NaN query, the zero query
        assert same(eng.searchWide(v, k, bits=bits), eng.searchArrays(v, k))
    with pytest.raises(EncodingError):
        eng.searchWide(q, 1025)
    assert same(eng.searchWide(q, 10, bits=bits), eng.searchArrays(q, 10))


def test_search_wide_after_mutations_equals_a_rebuilt_engine(wax):
    dims, n, k = 384, 6000, 65
    corpus = R.corpus_for(0, n + 500, dims)
    ids = np.arange(n + 500, dtype=np.uint64) * 5 + 3
    q = R.queries_for(dims, 1)[0]
    eng = make_engine(wax, 0, dims, corpus[:n], ids=ids[:n])
    for bits in (8, 16):
        eng.searchWide(q, k, bits=bits)                      # both mirrors exist before the store moves
    eng.addBatch(ids[n:], corpus[n:])
    eng.remove(int(ids[17]))
    eng.removeBatch(ids[1000:1400:3])
    keep = np.ones(n + 500, dtype=bool)
    keep[17] = keep[1000:1400:3] = False
    fresh = make_engine(wax, 0, dims, corpus[keep], ids=ids[keep])
    for bits in (8, 16):
        a, b = eng.searchWide(q, k, bits=bits, stats=True), fresh.searchWide(q, k, bits=bits, stats=True)
        assert same(a[:2], b[:2]) and same(a[:2], eng.searchArrays(q, k)) and a[2]["mirror"] == bits, (a[2], b[2])


def test_a_sharded_handle_answers_with_its_search(wax):
    dims, n, k = 384, 20005, 300
    many = wax.HIPVectorEngine(dimensions=dims, devices=[0] * 3)
    many.setTuning("shard_min_mb", 0)
    many.addBatch(np.arange(n, dtype=np.uint64), R.corpus_for(0, n, dims))
    for q in R.queries_for(dims, 2):
        ids, scores, st = many.searchWide(q, k, stats=True)
        assert same((ids, scores), many.searchArrays(q, k)) and st["mirror"] == 0 and st["certified"] == 0, st
