"""The timeline lane on the device (wax_amd/csrc/timeline.hip; wax_hip_timeline / _device / _probe) against the restatement of
TimelineQuery.filter in tests/timeline_ref.py. Every answer is array_equal to the model: ids, timestamps, count and padding.

Through the probe the selection runs with 1, 2 and 3 workgroups on 257, 4 097 and 20 000 rows, so that one workgroup walks dozens of
tiles and cuts its buffer repeatedly; through an engine the lane follows the store across mutations; the device form is a lane of the
device fusion. The dimension is irrelevant to the lane: every store is 64-d."""
import numpy as np
import pytest

import timeline_ref as ref

pytestmark = pytest.mark.gpu
DIMS = 64


@pytest.fixture(scope="module")
def wax():
    import wax_amd
    if not wax_amd.HIPVectorEngine.isAvailable():
        pytest.skip("no gfx950 device")
    return wax_amd


def _range(after, before):
    return None if after is None and before is None else (after, before)


# ---- through the probe ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ref.CASES, ids=lambda c: c.name)
def test_probe_equals_model(wax, case):
    ts, fl, ids = ref.columns(case)
    exp_ids, exp_ts = ref.expected(case)
    for grid in ref.GRIDS + (0,):                               # 0: the product's own grid
        got_ids, got_ts, n = wax.timelineProbe(ts, fl, ids, case.limit, case.newest, _range(case.after, case.before), case.deny, grid=grid)
        assert n == case.count == len(exp_ids), grid
        assert np.array_equal(got_ids, ref.padded(exp_ids, case.limit)), grid
        assert np.array_equal(got_ts[:n], exp_ts) and not got_ts[n:].any(), grid


# ---- through an engine ------------------------------------------------------------------------------------------------------

class Store:
    """An engine and what the test knows of it: frame id -> (timestamp, flags)."""

    def __init__(self, wax, devices=None):
        self.eng = wax.HIPVectorEngine(dimensions=DIMS, devices=devices)
        self.attrs = {}
        self.rng = np.random.default_rng(5)

    def vectors(self, n):
        return self.rng.standard_normal((n, DIMS)).astype(np.float32)

    def add(self, ids):
        ids = np.asarray(ids, dtype=np.uint64)
        self.eng.addBatch(ids, self.vectors(len(ids)))
        for i in ids.tolist():
            self.attrs.setdefault(i, (0, 0))                     # an appended row is (0, 0); an upsert keeps its row's attributes

    def set(self, ids, ts, fl):
        assert self.eng.setAttributes(ids, ts, fl) == len(ids)
        for i, t, f in zip(np.asarray(ids).tolist(), np.asarray(ts).tolist(), np.asarray(fl).tolist()):
            self.attrs[i] = (t, f)

    def check(self, queries):
        ids = np.fromiter(self.attrs.keys(), dtype=np.uint64, count=len(self.attrs))
        ts = np.array([v[0] for v in self.attrs.values()], dtype=np.int64)
        fl = np.array([v[1] for v in self.attrs.values()], dtype=np.uint32)
        assert self.eng.count == len(ids)
        out = []
        for limit, newest, after, before, deny in queries:
            exp = ref.timeline_model(ts, fl, ids, limit, newest, after, before, deny)
            got = self.eng.timeline(limit, newest, _range(after, before), deny)
            assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]), (limit, newest, after, before, deny)
            out.append(got)
        return out


QUERIES = ((30, True, None, None, 0), (300, False, None, None, 0),
           (1000, True, -2, 3, ref.FLAG_DELETED | ref.FLAG_SUPERSEDED), (4096, False, 0, None, ref.FLAG_SURROGATE))


def _attributes(rng, n):
    ts = rng.integers(-4, 5, size=n).astype(np.int64)            # nine timestamps: ties everywhere
    fl = rng.choice(np.array([0, 0, 0, ref.FLAG_DELETED, ref.FLAG_SUPERSEDED, ref.FLAG_SURROGATE, 0x100], dtype=np.uint32), size=n)
    return ts, fl


@pytest.mark.parametrize("n", [1, 255, 256, 257, 70_000])
def test_engine_follows_the_store(wax, n):
    rng = np.random.default_rng(n)
    s = Store(wax)
    assert s.eng.timeline(30)[0].size == 0                       # an empty engine
    ids = (rng.permutation(n).astype(np.uint64) * 3 + 7)         # frame order is not row order
    s.add(ids)
    s.check(QUERIES)                                             # attributes never set: every row (0, 0), every comparison a tie
    ts, fl = _attributes(rng, n)
    s.set(ids, ts, fl)
    s.check(QUERIES)
    new = np.arange(5, dtype=np.uint64) * 3 + 8                  # ids between the old ones
    s.add(new)                                                   # appended after setAttributes: (0, 0)
    s.eng.add(2, s.vectors(1)[0])                                # a single add is staged until the next reader
    s.attrs[2] = (0, 0)
    s.check(QUERIES)
    s.add(ids[:3])                                               # upserts: the rows keep their attributes
    s.check(QUERIES[:2])
    s.eng.remove(int(ids[0]))
    del s.attrs[int(ids[0])]
    s.check(QUERIES[:2])
    if n > 16:
        gone = ids[1:n:max(1, n // 9)]
        assert s.eng.removeBatch(gone) == len(gone)
        for i in gone.tolist():
            del s.attrs[i]
        s.check(QUERIES)
    cap = 64                                                     # WAX_HIP_INITIAL_RESERVE, doubled until the rows fit
    while cap < s.eng.count:
        cap *= 2
    grown = np.arange(cap - s.eng.count + 10, dtype=np.uint64) * 3 + 9   # past the capacity: the store and its columns move
    s.add(grown)
    m = min(50, len(grown))
    s.set(grown[:m], np.full(m, 4, dtype=np.int64), np.zeros(m, dtype=np.uint32))
    s.check(QUERIES)
    ticket = s.eng.submit(s.vectors(1)[0], 5)                    # the thread holds the shared lock through an uncollected ticket
    held = s.check(QUERIES[:1])
    s.eng.collect(ticket, 5)
    assert np.array_equal(s.check(QUERIES[:1])[0][0], held[0][0])
    for limit in (0, -1, -2**31):
        assert s.eng.timeline(limit)[0].size == 0
    with pytest.raises(wax.WaxError):
        s.eng.timeline(ref.MAX_LIMIT + 1)
    s.eng.deserialize(s.eng.serialize())                         # the columns are dropped
    s.attrs = {i: (0, 0) for i in s.attrs}
    s.check(QUERIES)
    s.eng.close()


@pytest.mark.parametrize("n", [257, 70_000])
def test_three_shards_on_one_device_equal_the_single_engine(wax, n):
    rng = np.random.default_rng(n + 1)
    one, many = Store(wax), Store(wax, devices=[0, 0, 0])
    ids = (rng.permutation(n).astype(np.uint64) * 3 + 7)
    ts, fl = _attributes(rng, n)
    many.eng.setTuning("shard_min_mb", 0)                        # spread from the first row: a 64-d store is far below the default block
    for s in (one, many):
        s.eng.reserve(n)
        s.add(ids)
    assert many.eng.shardCount == 3 and all(many.eng.shardInfo(g)[2] > 0 for g in range(3))
    for s in (one, many):
        a = s.check(QUERIES[:2])                                 # never-set attributes
        s.set(ids, ts, fl)
        b = s.check(QUERIES)
        s.eng.add(2, s.vectors(1)[0])
        s.attrs[2] = (0, 0)
        s.eng.remove(int(ids[n // 2]))
        del s.attrs[int(ids[n // 2])]
        c = s.check(QUERIES)
        s.answers = a + b + c
    for x, y in zip(one.answers, many.answers):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])
    assert many.eng.timeline(0)[0].size == 0
    one.eng.close()
    many.eng.close()


# ---- the device form --------------------------------------------------------------------------------------------------------

def test_device_form_equals_blocking_form_and_fuses_as_a_lane(wax):
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(21)
    n, k = 20_000, 30
    s = Store(wax)
    ids = (rng.permutation(n).astype(np.uint64) * 5 + 2)
    s.add(ids)
    ts, fl = _attributes(rng, n)
    s.set(ids, ts, fl)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for limit, newest, after, before, deny in QUERIES + ((ref.MAX_LIMIT, True, 4, 5, 0x100),):
        d_ids = torch.zeros(limit, dtype=torch.int64, device=dev)
        d_cnt = torch.full((1,), 99, dtype=torch.int32, device=dev)
        s.eng.timelineDevice(limit, d_ids, d_cnt, newest, _range(after, before), deny, stream=stream)
        torch.cuda.synchronize()
        exp = s.check([(limit, newest, after, before, deny)])[0]
        assert int(d_cnt.cpu()[0]) == len(exp[0])
        assert np.array_equal(d_ids.cpu().numpy().view(np.uint64), ref.padded(exp[0], limit))
    d_cnt = torch.full((1,), 99, dtype=torch.int32, device=dev)
    s.eng.timelineDevice(0, torch.zeros(1, dtype=torch.int64, device=dev), d_cnt, stream=stream)
    torch.cuda.synchronize()
    assert int(d_cnt.cpu()[0]) == 0
    # the lane in the fusion: searchBatch hits (pitch 2) and the timeline (stride = limit, pitch 1) on one stream, against the host
    # fusion of the host copies of the same two lists
    limit, deny = 300, ref.FLAG_DELETED | ref.FLAG_SUPERSEDED
    q = s.vectors(1)
    dq = torch.from_numpy(q).to(dev)
    hits = torch.empty((1, 40, 2), dtype=torch.int64, device=dev)
    s.eng.searchBatchHitsDevice(dq.data_ptr(), 1, k, hits.data_ptr(), 40, stream)
    lane = torch.zeros(limit, dtype=torch.int64, device=dev)
    lane_cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    s.eng.timelineDevice(limit, lane, lane_cnt, True, (-3, 4), deny, stream=stream)
    width = 512
    o_ids = torch.empty((1, width), dtype=torch.int64, device=dev)
    o_scores = torch.empty((1, width), dtype=torch.float32, device=dev)
    o_rank = torch.empty((1, width), dtype=torch.int32, device=dev)
    o_src = torch.empty((1, width), dtype=torch.int32, device=dev)
    o_cnt = torch.empty((1,), dtype=torch.int32, device=dev)
    lanes = [(hits.data_ptr() + 8, 0, 40, 2, 0.7), (lane.data_ptr(), lane_cnt.data_ptr(), limit, 1, 0.3)]
    wax.HybridSearch.rrfFusionBatchDevice(lanes, 1, 60, o_ids.data_ptr(), o_scores.data_ptr(), width, o_rank.data_ptr(), o_src.data_ptr(),
                                          o_cnt.data_ptr(), stream)
    torch.cuda.synchronize()
    vec_ids = s.eng.searchBatch(q, k)[0][0, :k]
    tl_ids = s.eng.timeline(limit, True, (-3, 4), deny)[0]
    assert len(vec_ids) == k and len(tl_ids) == limit
    host = wax.HybridSearch.rrfFusionArrays([(0.7, vec_ids), (0.3, tl_ids)], 60)
    m = int(o_cnt.cpu()[0])
    assert m == len(host[0]) <= width
    assert np.array_equal(o_ids.cpu().numpy().view(np.uint64)[0, :m], host[0])
    assert np.array_equal(o_scores.cpu().numpy()[0, :m], host[1])
    assert np.array_equal(o_rank.cpu().numpy().view(np.uint32)[0, :m], host[2])
    assert np.array_equal(o_src.cpu().numpy().view(np.uint32)[0, :m], host[3])
    s.eng.close()
