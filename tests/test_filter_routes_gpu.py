"""Every path of the single-query filtered / predicate search: which route ran and what it was charged.

The answers of these paths are pinned by test_predicate_gpu.py and the filtered cases of test_parity_gpu.py; this file pins the
ACCOUNTING of each call — the deltas of stats() (searches, rows_scanned, bytes_scanned) and of the route counters — against a numpy
model of the mask:
  gather       m rows, m * D * 4 bytes (m = passing rows);
  masked scan  live chunks * chunk rows, times D * 4 (a chunk is live when it holds a passing row); the other chunks are skipped;
  m = 0        nothing is charged; an allow-list of >= 4 096 ids (or none) still counts its device-side probe / predicate call.
"short_selects" stays 0 on every path here: the gather route selects with the radix selection, and the masked route's short selection
(64 < k <= 192) is enqueued but not counted — recorded as the code behaves, not derived.
Every answer is array_equal to searchFiltered(frameIds = the passing ids) of the one-device engine, computed once per
(store, mask, k, minScore); the three-shard handle is held to those same arrays.

Shapes: 4 099 x 384 (a list of 4 096 present ids exists; not a multiple of the 8-row chunk) and 1 027 x 768 (2-row chunks)."""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

B_HALF, B_BUT_ONE = 1 << 8, 1 << 9        # flag bits: a random half of the rows; every row but ONE
CHUNK = {384: 8, 768: 2}                  # rows per chunk of the masked scan
KS = (10, 65, 193)                        # merge_keys alone / select_short in front of it / beyond the fused lists: gathers
DEVICE_MIN = 4096                         # "filter_device_min": lists at least this long are probed on the device
STATS = ("searches", "rows_scanned", "bytes_scanned")
TUNING = ("filter_device_searches", "short_selects", "predicate_searches", "predicate_gather_searches", "predicate_masked_scans",
          "predicate_chunks_skipped")


@pytest.fixture(scope="module")
def wax(hip_lib):
    import wax_amd
    if hip_lib.wax_hip_device_count() == 0:
        pytest.skip("no HIP device on this host: the gpu-marked tests run on the MI355X box (pytest -m gpu)")
    assert hip_lib.wax_hip_available() == 1, "a HIP device is visible but it is not gfx950: the HIP path needs an MI355X"
    return wax_amd


class Store:
    """The same rows and attributes on a one-device engine and on a three-shard handle, and the numpy model of them."""

    def __init__(self, wax, n, dims, seed):
        self.n, self.dims = n, dims
        self.corpus = np.ascontiguousarray(oracle.gaussian_unit_rows(seed, n, dims), dtype=np.float32)
        self.ids = np.arange(n, dtype=np.uint64) * 3 + 7
        rng = np.random.default_rng(seed + 100)
        self.ts = np.arange(n, dtype=np.int64) - 500
        self.fl = np.where(rng.random(n) < 0.5, B_HALF, 0).astype(np.uint32) | np.uint32(B_BUT_ONE)
        self.one_row = n // 2 + 3
        self.fl[self.one_row] &= np.uint32(~B_BUT_ONE & 0xffffffff)
        self.range = (int(self.ts[13]), int(self.ts[n // 3 + 5]))      # a contiguous range with mid-chunk ends
        absent = np.arange(10 ** 9, 10 ** 9 + 20, dtype=np.uint64)
        short = self.ids[rng.choice(n, 300, replace=False)]
        self.lists = {"short": np.concatenate([short, absent, short[:15]])}
        if n >= DEVICE_MIN:
            long_ = self.ids[rng.choice(n, DEVICE_MIN, replace=False)]
            self.lists["long"] = np.concatenate([long_, absent, long_[:40]])
        self.query = oracle.gaussian_unit_queries(1, dims)[0]
        self.one = wax.HIPVectorEngine(metric=wax.VectorMetric(0), dimensions=dims)
        self.many = wax.HIPVectorEngine(metric=wax.VectorMetric(0), dimensions=dims, devices=[0, 0, 0])
        self.many.setTuning("shard_min_mb", 0)
        for eng in (self.one, self.many):
            eng.addBatch(self.ids, self.corpus)
            assert eng.setAttributes(self.ids, self.ts, self.fl) == n
        self._refs = {}

    def close(self):
        self.one.close()
        self.many.close()

    def mask(self, allow, timeRange, deny):
        m = (self.fl & np.uint32(deny)) == 0
        if timeRange is not None:
            m &= (self.ts >= timeRange[0]) & (self.ts < timeRange[1])
        if allow is not None:
            m &= np.isin(self.ids, self.lists[allow])
        return m

    def reference(self, allow, timeRange, deny, k, minScore=None):
        """searchFiltered(frameIds = the passing ids) on the one-device engine: computed once, never modified."""
        key = (allow, timeRange, deny, k, None if minScore is None else np.float32(minScore).tobytes())
        if key not in self._refs:
            ids, scores = self.one.searchFiltered(self.query, k, frameIds=self.ids[self.mask(allow, timeRange, deny)], minScore=minScore)
            ids.setflags(write=False)
            scores.setflags(write=False)
            self._refs[key] = (ids, scores)
        return self._refs[key]


@pytest.fixture(scope="module")
def s384(wax):
    s = Store(wax, 4_099, 384, seed=51)
    yield s
    s.close()


@pytest.fixture(scope="module")
def s768(wax):
    s = Store(wax, 1_027, 768, seed=52)
    yield s
    s.close()


def snapshot(eng):
    st = eng.stats()
    return np.array([int(getattr(st, f)) for f in STATS] + [int(eng.getTuning(c)) for c in TUNING], dtype=np.int64)


def expected_deltas(s, allow, timeRange, deny, route, k):
    """The numpy model of what one call is charged, in the order STATS + TUNING."""
    mask = s.mask(allow, timeRange, deny)
    m, row_bytes = int(mask.sum()), s.dims * 4
    predicate = timeRange is not None or deny != 0
    on_device = allow is not None and len(s.lists[allow]) >= DEVICE_MIN
    exp = dict.fromkeys(STATS + TUNING, 0)
    exp["predicate_searches"] = int(predicate)
    exp["filter_device_searches"] = int(on_device)
    if m == 0:
        return exp
    exp["searches"] = 1
    host_list = allow is not None and not on_device
    masked = predicate and not host_list and route == 2 and k <= 192
    if masked:
        c = CHUNK[s.dims]
        live = len(np.unique(np.flatnonzero(mask) // c))
        exp["predicate_masked_scans"] = 1
        exp["predicate_chunks_skipped"] = (s.n + c - 1) // c - live
        exp["rows_scanned"] = live * c
    else:
        exp["predicate_gather_searches"] = int(predicate)
        exp["rows_scanned"] = m
    exp["bytes_scanned"] = exp["rows_scanned"] * row_bytes
    return exp


def run_case(s, allow=None, timeRange=None, deny=0, route=1, ks=KS, minScore=None, ctx=""):
    frame_ids = None if allow is None else s.lists[allow]
    for eng in (s.one, s.many):
        eng.setTuning("predicate_route", route)
    try:
        for k in ks:
            ref = s.reference(allow, timeRange, deny, k, minScore)
            before = snapshot(s.one)
            got = s.one.searchFiltered(s.query, k, frameIds=frame_ids, minScore=minScore, timeRange=timeRange, denyFlags=deny)
            delta = dict(zip(STATS + TUNING, (snapshot(s.one) - before).tolist()))
            exp = expected_deltas(s, allow, timeRange, deny, route, k)
            print(f"{ctx} k {k}: {delta}")
            assert delta == exp, f"{ctx} k {k}: charged {delta}, the mask says {exp}"
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), f"{ctx} k {k}: differs from the allow-list reference"
            many = s.many.searchFiltered(s.query, k, frameIds=frame_ids, minScore=minScore, timeRange=timeRange, denyFlags=deny)
            assert np.array_equal(many[0], ref[0]) and np.array_equal(many[1], ref[1]), f"{ctx} k {k}: three shards differ"
    finally:
        for eng in (s.one, s.many):
            eng.setTuning("predicate_route", 0)


# name -> (allow-list, uses the time range, deny bits)
MASKS = {"random half": (False, B_HALF), "contiguous range": (True, 0), "single row": (False, B_BUT_ONE), "range and half": (True, B_HALF)}


@pytest.mark.parametrize("allow", ["short", "long"])
def test_allow_list_alone(s384, allow):
    assert (len(s384.lists[allow]) >= DEVICE_MIN) == (allow == "long")
    assert s384.mask(allow, None, 0).sum() == (300 if allow == "short" else DEVICE_MIN)     # absent and repeated ids add nothing
    run_case(s384, allow=allow, ctx=f"{allow} list")


def test_allow_list_alone_768(s768):
    run_case(s768, allow="short", ctx="768-d short list")


@pytest.mark.parametrize("route", [1, 2])
@pytest.mark.parametrize("name", list(MASKS))
def test_predicate_alone(s384, s768, name, route):
    for s in (s384, s768):
        use_range, deny = MASKS[name]
        tr = s.range if use_range else None
        m = s.mask(None, tr, deny)
        if name == "single row":
            assert m.sum() == 1 and m[s.one_row]
        if name == "contiguous range":
            assert m.sum() == s.n // 3 + 5 - 13
        run_case(s, timeRange=tr, deny=deny, route=route, ctx=f"{s.dims}-d {name}, route {route}")


@pytest.mark.parametrize("route", [1, 2])
@pytest.mark.parametrize("allow", ["short", "long"])
def test_predicate_and_allow_list(s384, allow, route):
    s = s384
    for name in ("random half", "contiguous range"):
        use_range, deny = MASKS[name]
        tr = s.range if use_range else None
        assert 0 < s.mask(allow, tr, deny).sum() < s.mask(allow, None, 0).sum()
        run_case(s, allow=allow, timeRange=tr, deny=deny, route=route, ctx=f"{allow} list and {name}, route {route}")


def test_predicate_and_short_list_768(s768):
    for route in (1, 2):
        run_case(s768, allow="short", deny=B_HALF, route=route, ctx=f"768-d short list and random half, route {route}")


@pytest.mark.parametrize("route", [1, 2])
def test_nothing_passes(s384, route):
    """m = 0 behind the counters of the steps that ran: the predicate call, the device-side probe of a long list."""
    s = s384
    for allow in (None, "short", "long"):
        tr = (int(s.ts[-1]) + 1, int(s.ts[-1]) + 2)
        assert s.mask(allow, tr, 0).sum() == 0
        run_case(s, allow=allow, timeRange=tr, route=route, ks=(10,), ctx=f"nothing passes, list {allow}, route {route}")


@pytest.mark.parametrize("route", [1, 2])
def test_min_score(s384, route):
    """A finite cut (an earlier answer's 5th score) keeps exactly the scores >= cut; a NaN cut keeps what no cut keeps."""
    s = s384
    for allow, deny in (("short", 0), ("long", 0), (None, B_HALF), ("short", B_HALF), ("long", B_HALF)):
        ctx = f"list {allow}, deny {deny:#x}, route {route}"
        full = s.reference(allow, None, deny, 65)
        cut = float(full[1][4])
        keep = full[1] >= np.float32(cut)
        assert 5 <= keep.sum() < 65
        cut_ref = s.reference(allow, None, deny, 65, minScore=cut)
        assert np.array_equal(cut_ref[0], full[0][keep]) and np.array_equal(cut_ref[1], full[1][keep]), ctx
        run_case(s, allow=allow, deny=deny, route=route, ks=(65,), minScore=cut, ctx=ctx + ", finite cut")
        nan_ref = s.reference(allow, None, deny, 65, minScore=float("nan"))
        assert np.array_equal(nan_ref[0], full[0]) and np.array_equal(nan_ref[1], full[1]), ctx
        run_case(s, allow=allow, deny=deny, route=route, ks=(65,), minScore=float("nan"), ctx=ctx + ", NaN cut")
