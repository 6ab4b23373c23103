"""Every row position of the store, required at rank 1 and at rank 2, on every batched route (run with -m gpu on an MI355X).

The batched pipelines — the filtering GEMM batch_gemm_rq_kernel with its 32-, 64- and 128-row tiles, padded LDS images, two and three
tile buffers, fixed shares, tail pool, clipped workgroup count, one to four query groups and split barrier; the LDS-tiled
batch_gemm_kernel; the slab pipeline; the shared exact pass scan_multi_kernel — are swept with the twin stores of
tests/batch_positions_ref.py: the queries are the stored rows themselves, in store order, in batches with a ragged last one, top_k 2,
and query i must answer [i, partner(i)]. A row the filter never scores, or scores from another row's bytes, is then the missing first or
second hit of a query of the sweep (tests/test_batch_positions_cpu.py, (d)); on the random corpora of the other tests it only has to lose.

Stores are drawn on the device by the recipe of batch_positions_ref.twin_store (a seeded torch.Generator), appended with
addBatchDevice, and copied to the host once for the float64 model; queries and hits stay on the device, nothing is uploaded per batch.
Per case (batch_positions_ref.CASES):
  1. ids [i, partner(i)] and count 2 for every query, compared on the device;
  2. every score within helpers.SCORE_TOL of the float64 model;
  3. 32 queries — rows 0 and N - 1, the rows around the pool's first tile, the ragged last tile, the rows on each side of a shard
     boundary, random ones — bit for bit what searchArrays answers;
  4. the route the case claims, through the counters, and on the certified routes at most ceil(N / 1000) queries of the sweep answered
     by an exact pass over the f32 store ("batch_fallbacks", and the queries of a ragged last batch below 16 that the cost model sends
     to single scans: "batch_queries" short of the sweep). The device-side full retry re-scores the filter's survivors only and is
     not counted. The cap is a condition, not a measurement: such a query could hide a row the filter missed; the CPU test's (c)
     shows that the certificate never asks for one on these stores;
  5. pool cases: the sweep under "batch_dyn_tail" 0 gives the same hits, array_equal.

"exact-l2-100" is listed by the table under the shared exact passes, but scan_multi_kernel serves the specialised dimensions only: at
100 dimensions "batch_mode" 0 answers every query of a batch by its own scan inside exact_scan_queries, and that is what the case
asserts ("batch_multi_passes" does not move, one search per query).

Out of scope: the pace gate of the filtering GEMM. It engages above 1 024 tiles per workgroup of a launch with several query groups —
millions of rows per sweep — and no store here reaches it.

Measured on an MI355X, counter deltas over one sweep (exact = queries of the sweep answered by an exact pass over the f32 store, cap =
ceil(N / 1000); retries = "batch_retries", device-side and host full retries, not counted against the cap; the handle's counters are
sums over its three shards). No query of any certified route fell back; the three exact queries of clipped-cos384 are its ragged last
batch of three, which the cost model sends to one shared exact pass. The whole file takes 10 s, its slowest case (pool-cos384, 2 x
1 537 blocking batches over the 302 MB mirror) 3.3 s.

  case                 rows     per batch  batch_queries  onepass_queries  batch_fallbacks  retries  multi passes  exact  cap
  pool-cos384          393 253  256        393 253        393 253          0                0        0             0      394
  pool-cos768          196 627  256        196 627        196 627          0                0        0             0      197
  fixed-cos128         40 037   256        40 037         40 037           0                0        0             0      41
  fixed-cos256         40 037   256        40 037         40 037           0                0        0             0      41
  fixed-cos384         40 037   256        40 037         40 037           0                0        0             0      41
  fixed-cos512         40 037   256        40 037         40 037           0                0        0             0      41
  fixed-cos768         40 037   256        40 037         40 037           0                0        0             0      41
  fixed-dot384         40 037   256        40 037         40 037           0                0        0             0      41
  clipped-cos384       4 099    256        4 096          4 096            0                0        1             3      5
  groups2-cos384       40 037   512        40 037         40 037           0                0        0             0      41
  groups3-cos384       40 037   768        40 037         40 037           0                0        0             0      41
  groups4-cos384       40 037   1 024      40 037         40 037           0                0        0             0      41
  groups2-cos768       40 037   512        40 037         40 037           0                0        0             0      41
  groups3-cos768       40 037   768        40 037         40 037           0                0        0             0      41
  groups4-cos768       40 037   1 024      40 037         40 037           0                0        0             0      41
  split-cos384         40 037   256        40 037         40 037           0                0        0             0      41
  split-cos768         40 037   256        40 037         40 037           0                0        0             0      41
  tiled-cos64          65 613   256        65 613         65 613           0                0        0             0      66
  tiled-dot192         65 613   256        65 613         65 613           0                0        0             0      66
  tiled-l2-384         65 613   256        65 613         65 613           0                0        0             0      66
  slab-small-slabs     20 011   256        20 011         0                0                0        0             0      21
  slab-default-slabs   20 011   256        20 011         0                0                0        0             0      21
  slab-below-floor     3 001    256        3 001          0                0                0        0             0      4
  exact-cos384         5 003    256        0              0                0                0        313           5 003  -
  exact-l2-100         5 003    256        0              0                0                0        0             5 003  -
  handle-cos384        40 037   256        120 111        120 111          0                0        0             0      41"""
import numpy as np
import pytest

import batch_positions_ref as P
from helpers import SCORE_TOL

pytestmark = pytest.mark.gpu

KEY_PAD = np.iinfo(np.int64).max
COUNTERS = ("batch_queries", "onepass_queries", "batch_fallbacks", "batch_multi_passes", "batch_multi_queries", "batch_retries")
BIT_SAMPLE = 32
POISON = -2                                  # what the hit buffer holds before a sweep: no stale answer survives into the next one


@pytest.fixture(scope="module")
def wax(hip_lib):
    import wax_amd
    if hip_lib.wax_hip_device_count() == 0:
        pytest.skip("no HIP device on this host: the gpu-marked tests run on the MI355X box (pytest -m gpu)")
    assert hip_lib.wax_hip_available() == 1, "a HIP device is visible but it is not gfx950: the HIP path needs an MI355X"
    return wax_amd


class Store:
    """A twin store on device 0 (frameId = row) in an engine — or a handle of `shards` shards —, its rows kept on the device as the
    sweep's queries, and the float64 model of the sweep's answers computed once from the one host copy."""

    def __init__(self, wax, metric, dims, n, shards=0):
        import torch
        self.torch, self.wax = torch, wax
        self.metric, self.dims, self.n, self.shards = metric, dims, n, max(shards, 1)
        dev = torch.device("cuda", 0)
        g = torch.Generator(device=dev)
        g.manual_seed(P.store_seed(metric, dims, n))
        h = n // 2
        unit = torch.nn.functional.normalize
        base = unit(torch.randn((h, dims), generator=g, device=dev, dtype=torch.float32), dim=1)
        noise = torch.randn((h, dims), generator=g, device=dev, dtype=torch.float32) * (P.SIGMA / float(np.sqrt(dims)))
        parts = [base, unit(base + noise, dim=1)]
        if n % 2:
            parts.append(unit(torch.randn((1, dims), generator=g, device=dev, dtype=torch.float32), dim=1))
        rows = torch.cat(parts, dim=0)
        if metric == P.DOT:
            rows = rows * P.DOT_SCALE
        self.rows = rows.contiguous()
        del base, noise, parts
        if shards:
            self.eng = wax.HIPVectorEngine(metric=wax.VectorMetric(metric), dimensions=dims, devices=[0] * shards)
            self.eng.setTuning("shard_min_mb", 0)
        else:
            self.eng = wax.HIPVectorEngine(metric=wax.VectorMetric(metric), dimensions=dims)
        self.eng.reserve(n)
        self.eng.addBatchDevice(np.arange(n, dtype=np.uint64), self.rows)
        assert self.eng.count == n
        host = self.rows.cpu().numpy()
        cos = P.pair_cosines(host)                                    # (a) of the CPU test, on the rows the device drew
        assert P.PAIR_COS_MIN <= cos.min() and cos.max() <= P.PAIR_COS_MAX, (cos.min(), cos.max())
        ids, scores = P.expected(host, metric)
        del host
        self.partner = P.partner(n)
        self.exp_ids = torch.from_numpy(ids).to(dev)
        self.exp_scores = torch.from_numpy(scores).to(dev)
        self.out = torch.empty((n, P.K, 2), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()

    def shard_bases(self):
        return [self.eng.shardInfo(g)[1] for g in range(self.shards)] if self.shards > 1 else []

    def counters(self):
        c = {k: self.eng.getTuning(k) for k in COUNTERS}
        c["searches"] = int(self.eng.stats().searches)
        return c

    def sweep(self, nq, pipelined=False):
        """The stored rows as queries, in store order, nq per batch: hits [n, 2, 2] (key, frame id) on the device."""
        torch, eng, n, dims = self.torch, self.eng, self.n, self.dims
        self.out.fill_(POISON)
        torch.cuda.synchronize()
        stream = torch.cuda.current_stream().cuda_stream
        q0, o0 = self.rows.data_ptr(), self.out.data_ptr()
        tickets = []
        for lo in range(0, n, nq):
            m = min(nq, n - lo)
            args = (q0 + lo * dims * 4, m, P.K, o0 + lo * P.K * 16, P.K, stream)
            if pipelined:                                            # two batches in flight
                if len(tickets) == 2:
                    eng.searchBatchCollectDevice(tickets.pop(0))
                tickets.append(eng.searchBatchSubmitDevice(*args))
            else:
                eng.searchBatchHitsDevice(*args)
        for t in tickets:
            eng.searchBatchCollectDevice(t)
        torch.cuda.synchronize()
        return self.out.clone()

    def scores_of(self, keys):
        """Scores of hit keys on the device: the distance is the key's upper word through order_bits' inverse (common.h), the score
        hits_to_results' (1 - d under cosine, -d otherwise), in f32."""
        torch = self.torch
        o = (keys >> 32).to(torch.int32)
        d = (o ^ ((o >> 31) & 0x7fffffff)).view(torch.float32)
        return (1.0 - d) if self.metric == P.COS else -d

    def where(self, bad, case):
        """The failing rows with their place in the filter's walk: what a message needs to name the tile, workgroup and side of the pool."""
        rows = self.torch.nonzero(bad).flatten()[:12].cpu().numpy().tolist()
        tr = P.tile_rows(self.metric, self.dims)
        per_group = P.workgroups_per_group(self.metric, self.dims, self.n, case["nq"])
        pool = P.pool_first_row(self.metric, self.dims, self.n, case["nq"])
        return [{"row": r, "tile": r // tr, "row_in_tile": r % tr, "workgroup": (r // tr) % per_group, "position": (r // tr) // per_group,
                 "in_pool": pool is not None and r >= pool, "batch": r // case["nq"], "query_in_batch": r % case["nq"]} for r in rows]

    def wrong(self, hits):
        """Per query of the sweep, on the device: (count is not 2, rank 1 is not the row itself, rank 2 is not the twin)."""
        keys, fids = hits[:, :, 0], hits[:, :, 1]
        paired = self.exp_ids[:, 1] >= 0
        return ((keys != KEY_PAD).sum(dim=1) != P.K, fids[:, 0] != self.exp_ids[:, 0], paired & (fids[:, 1] != self.exp_ids[:, 1]))

    def check(self, hits, case):
        torch = self.torch
        keys = hits[:, :, 0]
        for what, bad in zip(("count is not 2", "rank 1 is not the row itself", "rank 2 is not the twin"), self.wrong(hits)):
            assert not bool(bad.any()), (case["id"], what, int(bad.sum()), self.where(bad, case))
        err = (self.scores_of(keys).double() - self.exp_scores).abs()
        err = torch.where(torch.isnan(self.exp_scores), torch.zeros_like(err), err)      # the lone row's second hit: not checked
        bad = (err > SCORE_TOL).any(dim=1)
        print(f"[{case['id']}] max |score - float64 model| {float(err.max()):.3g}")
        assert not bool(bad.any()), (case["id"], "score", float(err.max()), self.where(bad, case))

    def check_bits(self, hits, case):
        """BIT_SAMPLE queries of the sweep against searchArrays on the same engine, bit for bit."""
        sample = P.bit_sample(self.metric, self.dims, self.n, case["nq"], self.shard_bases(), BIT_SAMPLE)
        assert len(sample) == BIT_SAMPLE and sample[0] == 0 and sample[-1] == self.n - 1
        idx = self.torch.from_numpy(sample).to(self.rows.device)
        queries = self.rows[idx].cpu().numpy()
        got = hits[idx].cpu().numpy()
        for j, r in enumerate(sample):
            b_ids, b_scores = self.wax.HIPVectorEngine.hitsToResults(self.wax.VectorMetric(self.metric), got[j])
            s_ids, s_scores = self.eng.searchArrays(queries[j], P.K)
            assert np.array_equal(b_ids, s_ids) and np.array_equal(b_scores, s_scores), (case["id"], int(r), b_ids, s_ids, b_scores, s_scores)

    def close(self):
        self.eng.close()


@pytest.fixture(scope="module")
def stores(wax):
    """One store per (metric, dims, rows, shards) of the table, built when first asked for and kept for the cases that share it."""
    built = {}

    def get(metric, dims, n, shards=0):
        key = (metric, dims, n, shards)
        if key not in built:
            built[key] = Store(wax, metric, dims, n, shards)
        return built[key]

    yield get
    for st in built.values():
        st.close()


def _assert_route(case, st, d):
    """The counters of one sweep (deltas `d`) say that the route of the case answered it; returns the queries of the sweep that an
    exact pass over the f32 store answered."""
    n, nq, route, shards = st.n, case["nq"], case["route"], st.shards
    tail = n % nq
    batches = [min(nq, n - lo) for lo in range(0, n, nq)]
    if route == P.EXACT:
        assert d["batch_queries"] == 0 and d["onepass_queries"] == 0 and d["batch_fallbacks"] == 0, d
        assert d["searches"] == n, d
        if st.eng.getTuning("batch_multi_group") >= 2:
            assert st.eng.getTuning("batch_multi_group") == 16
            assert d["batch_multi_queries"] == n and d["batch_multi_passes"] == sum(-(-m // 16) for m in batches), d
        else:                                   # no shared pass at this dimension: one scan per query
            assert st.dims == 100 and d["batch_multi_queries"] == 0 and d["batch_multi_passes"] == 0, d
        return n
    # a batch of 16 queries or more always takes the pipeline; a ragged last batch below 16 is the cost model's to place
    through = (n, n - tail) if 0 < tail < 16 else (n,)
    assert d["batch_queries"] in [shards * t for t in through], (d, through)
    if route == P.SLAB:
        assert d["onepass_queries"] == 0, d
    else:
        assert d["onepass_queries"] == d["batch_queries"], d
    exact = (n - d["batch_queries"] // shards) + d["batch_fallbacks"]
    assert d["batch_multi_queries"] <= exact, d          # the shared exact passes serve those queries and nobody else
    return exact


def test_a_lost_row_position_fails_the_sweep_at_that_row_and_its_twin(wax):
    """(d) of the CPU test, seen through the engine: take one row position out of the store (an upsert puts a stranger in its place;
    the sweep still asks with the row that was there) and the comparison of the sweep names exactly that row's query and its twin's —
    the lone last row: its own alone. Put back, the sweep is clean again. On the smallest one-pass store, on a store of its own."""
    st = Store(wax, P.COS, 384, P.N_CLIP)
    try:
        n, h = st.n, st.n // 2
        rng = np.random.default_rng(5)
        for r in (0, h + 7, n - 1):
            original = st.rows[r].cpu().numpy()
            stranger = rng.standard_normal(384).astype(np.float32)
            st.eng.add(r, stranger / np.linalg.norm(stranger))
            count_bad, first_bad, second_bad = st.wrong(st.sweep(256))
            assert not bool(count_bad.any())
            flagged = st.torch.nonzero(first_bad | second_bad).flatten().cpu().numpy().tolist()
            assert flagged == sorted({r, int(st.partner[r])} - {-1}), (r, flagged)
            assert st.torch.nonzero(first_bad).flatten().cpu().numpy().tolist() == [r]
            st.eng.add(r, original)
            assert not any(bool(bad.any()) for bad in st.wrong(st.sweep(256))), r
        assert st.eng.count == n
    finally:
        st.close()


@pytest.mark.parametrize("case", P.CASES, ids=lambda c: c["id"])
def test_sweep(wax, stores, case):
    metric, dims, n, nq, route = case["metric"], case["dims"], case["n"], case["nq"], case["route"]
    st = stores(metric, dims, n, P.HANDLE_SHARDS if route == P.HANDLE else 0)
    eng = st.eng
    # what the case claims about the engine it runs on
    assert eng.getTuning("batch_dyn_tail") == 1 and eng.getTuning("batch_rega") == 1 and eng.getTuning("batch_onepass") == 1
    assert eng.getTuning("batch_mode") == 1 and eng.getTuning("batch_slab_mb") == 64 and eng.getTuning("batch_min") == 1
    assert (P.pool_first_row(metric, dims, n, nq) is not None) == (route == P.POOL)
    if route == P.HANDLE:
        assert eng.getTuning("shards") == P.HANDLE_SHARDS
        bases = np.array(st.shard_bases())
        assert bases[0] == 0 and np.all(np.diff(bases) > 0) and bases[-1] < n
        shard_of = np.searchsorted(bases, np.arange(n), side="right") - 1
        paired = st.partner >= 0
        assert np.all(shard_of[paired] != shard_of[st.partner[paired]]), "twins fall in different shards"
    old = {key: eng.getTuning(key) for key, _ in case["tuning"]}
    try:
        for key, value in case["tuning"]:
            eng.setTuning(key, value)
            assert eng.getTuning(key) == value
        before = st.counters()
        hits = st.sweep(nq, case["pipelined"])
        after = st.counters()
        d = {k: after[k] - before[k] for k in after}
        exact = _assert_route(case, st, d)
        print(f"\n[{case['id']}] {P.METRIC_NAME[metric]} {dims} x {n}, {nq} per batch: exact {exact} (cap {P.fallback_cap(n)}), "
              f"fallbacks {d['batch_fallbacks']}, retries {d['batch_retries']}, multi passes {d['batch_multi_passes']}, "
              f"batch queries {d['batch_queries']}, one-pass {d['onepass_queries']}")
        st.check(hits, case)
        st.check_bits(hits, case)
        if route in P.CERTIFIED_ROUTES:
            assert exact <= P.fallback_cap(n), (case["id"], exact, d)
        if route == P.POOL:
            eng.setTuning("batch_dyn_tail", 0)
            try:
                fixed = st.sweep(nq)
            finally:
                eng.setTuning("batch_dyn_tail", 1)
            assert bool(st.torch.equal(fixed, hits)), "fixed shares and the pool disagree"
    finally:
        for key, value in old.items():
            eng.setTuning(key, value)
