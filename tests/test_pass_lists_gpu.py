"""The selection frame of a mirror pass (mirror_pass.h: PassLists — the wave lists, their first prune and the prunes behind the
sorted prefix after it, the final prunes, the workgroup rank merge) on made-up keys through wax_hip_mirror_lists_probe, held with
array_equal to the host model of tests/pass_lists_ref.py: every workgroup keeps, for every query, the 64 smallest keys it was
offered. Every case runs at 1, 2, 3 and 4 queries per pass; member q of a case is the case's q-th stream set. The cases are also
those a threshold shared inside a workgroup would have to survive (keys that arrive late, in one wave, below everything seen).

And once on the real path: a 70 000 x 384 store at "grid_blocks" 8 (every wave prunes repeatedly), every query alone and as a member of
passes of 2, 3 and 4 on the 8-bit code mirror — the same answer every time, the exact f32 scan's, out of the 64 smallest of the
pass's own keys (wax_hip_mirror8_keys)."""
import ctypes

import numpy as np
import pytest

import oracle
import pass_lists_ref as P

pytestmark = pytest.mark.gpu

NQS = (1, 2, 3, 4)


@pytest.fixture(scope="module")
def wax(hip_lib):
    import wax_amd
    if hip_lib.wax_hip_device_count() == 0:
        pytest.skip("no HIP device on this host: the gpu-marked tests run on the MI355X box (pytest -m gpu)")
    assert hip_lib.wax_hip_available() == 1, "a HIP device is visible but it is not gfx950: the HIP path needs an MI355X"
    return wax_amd


def run(hip_lib, keys, grid):
    keys = np.ascontiguousarray(keys, dtype=np.int64)
    nq, n_slots = keys.shape
    out = np.zeros((nq, grid, P.KP), dtype=np.int64)
    p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))   # noqa: E731
    rc = hip_lib.wax_hip_mirror_lists_probe(p(keys), nq, n_slots, grid, p(out))
    assert rc == 0, rc
    return out


def check(hip_lib, members, grid):
    """members: four [n_slots] key arrays; a pass of nq runs the first nq"""
    members = [np.asarray(m, dtype=np.int64) for m in members]
    assert len(members) == 4 and len({len(m) for m in members}) == 1
    for m in members:
        live = m[m != P.PAD]
        assert len(np.unique(live)) == len(live), "the frame's keys are unique"
    for nq in NQS:
        keys = np.stack(members[:nq])
        want = P.partials(keys, grid)
        got = run(hip_lib, keys, grid)
        assert np.array_equal(got, want), f"{nq} queries, {grid} workgroups: first difference at {np.argwhere(got != want)[:4].tolist()}"


def rows_of(n):
    return np.arange(n, dtype=np.int64)


def random_keys(seed, n_slots):
    words = np.random.default_rng(seed).integers(-(1 << 30), 1 << 30, size=n_slots)
    return P.make_key(words, rows_of(n_slots))


def descending(n_slots, grid):
    """strictly descending along every wave's walk (and over the whole launch): every offered key passes every threshold"""
    return P.make_key((1 << 30) - rows_of(n_slots), rows_of(n_slots))


def ascending(n_slots):
    return P.make_key(rows_of(n_slots) - (1 << 20), rows_of(n_slots))


@pytest.mark.parametrize("grid", [1, 2, 3])
@pytest.mark.parametrize("per_wave", [40, 300, 700])
def test_random_keys(wax, hip_lib, per_wave, grid):
    n_slots = per_wave * P.WAVES * grid + 5              # (no multiple of a tile)
    check(hip_lib, [random_keys(100 * per_wave + 10 * grid + q, n_slots) for q in range(4)], grid)


@pytest.mark.parametrize("grid", [1, 3])
def test_descending_keys_pass_every_threshold(wax, hip_lib, grid):
    n_slots = 700 * P.WAVES * grid
    d = descending(n_slots, grid)
    check(hip_lib, [d, d - (1 << 40), d + (1 << 40), d - (1 << 41)], grid)


@pytest.mark.parametrize("grid", [1, 3])
def test_ascending_keys_stop_after_the_first_lists(wax, hip_lib, grid):
    n_slots = 700 * P.WAVES * grid + 3
    a = ascending(n_slots)
    check(hip_lib, [a, a + (1 << 40), a - (1 << 40), a + (1 << 41)], grid)


def test_equal_words_everywhere_leave_the_row_to_order(wax, hip_lib):
    n_slots = 300 * P.WAVES * 2 + 9
    rng = np.random.default_rng(5)
    members = [P.make_key(np.full(n_slots, 1000 + q), rng.permutation(n_slots)) for q in range(4)]
    check(hip_lib, members, 2)


@pytest.mark.parametrize("where", ["first_wave", "last_wave", "last_iteration"])
def test_all_of_the_best_in_one_place(wax, hip_lib, where):
    """the workgroup's 64 best in one wave's stream — at its start or its end — or, last_iteration, spread over the four waves' last
    tiles: they arrive behind every prune but the final one and must displace all that the lists hold"""
    grid, tiles = 2, 40
    nwaves = P.WAVES * grid
    members = []
    for q in range(4):
        rng = np.random.default_rng(40 + q)
        streams = [list(P.make_key(rng.integers(1 << 20, 1 << 30, size=tiles * P.TILE), (w * tiles * P.TILE + rows_of(tiles * P.TILE))))
                   for w in range(nwaves)]
        best = P.make_key(-(1 << 20) - rows_of(64) * 3 - q, (1 << 24) + rows_of(64))
        for b in range(grid):
            waves = range(b * P.WAVES, (b + 1) * P.WAVES)
            if where == "first_wave":
                streams[waves[0]][:64] = list(best + b)
            elif where == "last_wave":
                streams[waves[-1]][-64:] = list(best + b)
            else:
                for j, w in enumerate(waves):
                    streams[w][-16:] = list(best[16 * j:16 * j + 16] + b)
        members.append(P.from_streams(streams, grid))
    check(hip_lib, members, grid)


@pytest.mark.parametrize("offered", [0, 1, 63, 64, 65])
def test_few_offered_keys(wax, hip_lib, offered):
    """workgroup 0 is offered `offered` keys per query over 200 slots per wave, workgroup 1 plenty, workgroup 2 none at all"""
    grid = 3
    n_slots = 200 * P.WAVES * grid
    wg = P.workgroup_of_slots(n_slots, grid)
    members = []
    for q in range(4):
        keys = random_keys(70 + q, n_slots)
        rng = np.random.default_rng(80 + q)
        first = np.flatnonzero(wg == 0)
        keep = rng.choice(first, size=offered, replace=False)
        hole = np.ones(n_slots, dtype=bool)
        hole[keep] = False
        hole[wg == 1] = False
        keys[hole] = P.PAD
        members.append(keys)
    check(hip_lib, members, grid)


@pytest.mark.parametrize("admitted", [111, 112, 113, 128])
def test_counts_at_the_edge_of_room(wax, hip_lib, admitted):
    """one wave with `admitted` keys in its list in front of an iteration (descending: all admitted; room(16) prunes above 112), then
    three more tiles: the prune that follows — the list's first, the general one — takes 113 to 128 keys, the one behind it runs
    on the sorted prefix; the other waves idle or busy by member"""
    grid = 1
    members = []
    for q in range(4):
        n = admitted + 48
        stream0 = list(P.make_key(-(1 << 20) - 7 * rows_of(n) - q, rows_of(n)))      # (below every other wave's keys)
        stream0[admitted:admitted] = [P.PAD] * ((-admitted) % P.TILE)           # the iteration that follows begins on a tile
        others = [list(P.make_key((1 << 28) + rows_of(400) * (5 + w), (w << 20) + rows_of(400))) if (q + w) % 2 else [] for w in (1, 2, 3)]
        members.append(P.from_streams([stream0] + others, grid))
    n_slots = max(len(m) for m in members)
    members = [np.concatenate([m, np.full(n_slots - len(m), P.PAD, dtype=np.int64)]) for m in members]
    check(hip_lib, members, grid)


def test_members_whose_streams_differ(wax, hip_lib):
    """member 0 prunes all the way (descending), member 1 is offered nothing for 300 slots per wave and random keys after, member 2
    ascends (its lists stay at 64: no final prune), member 3 holds a few keys only: an iteration's prunes meet lists above, at and
    below k, sorted and not"""
    grid = 2
    per_wave = 640
    n_slots = per_wave * P.WAVES * grid
    m0 = descending(n_slots, grid)
    m1 = random_keys(9, n_slots)
    m1[:300 * P.WAVES * grid] = P.PAD
    m2 = ascending(n_slots)
    m3 = random_keys(11, n_slots)
    m3[np.random.default_rng(12).random(n_slots) > 0.004] = P.PAD
    check(hip_lib, [m0, m1, m2, m3], grid)
    check(hip_lib, [m2, m0, m3, m1], grid)
    check(hip_lib, [m3, m2, m1, m0], grid)


def test_always_candidates(wax, hip_lib):
    """rows whose key is -inf (NaN and unbounded rows): fewer than 64, and more than a list holds"""
    grid = 2
    n_slots = 300 * P.WAVES * grid + 11
    members = []
    for q, share in enumerate((0.01, 0.2, 0.6, 1.0)):
        keys = random_keys(20 + q, n_slots)
        always = np.random.default_rng(30 + q).random(n_slots) < share
        keys[always] = P.make_key(np.full(int(always.sum()), P.NEG_INF_WORD), np.flatnonzero(always))
        members.append(keys)
    check(hip_lib, members, grid)
    check(hip_lib, members[::-1], grid)


def test_holes_of_whole_iterations(wax, hip_lib):
    """masked-style: whole tiles of holes, other tiles for every member and every other row for member 3"""
    grid = 3
    n_slots = 500 * P.WAVES * grid + 7
    tile = np.arange(n_slots) // P.TILE
    members = []
    for q in range(4):
        keys = random_keys(50 + q, n_slots)
        if q < 3:
            keys[(tile % (q + 2)) != 0] = P.PAD
        else:
            keys[1::2] = P.PAD
        members.append(keys)
    check(hip_lib, members, grid)


def test_the_probe_refuses_what_it_cannot_run(hip_lib):
    from wax_amd import _abi
    keys, out = np.zeros(16, dtype=np.int64), np.zeros(8 * 4 * 64, dtype=np.int64)
    p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))   # noqa: E731
    for nq, n_slots, grid in ((0, 16, 1), (5, 16, 1), (1, 0, 1), (1, (1 << 24) + 1, 1), (1, 16, 0), (1, 16, 9)):
        assert hip_lib.wax_hip_mirror_lists_probe(p(keys), nq, n_slots, grid, p(out)) == _abi.ERR_INVALID_ARGUMENT, (nq, n_slots, grid)
    assert hip_lib.wax_hip_mirror_lists_probe(None, 1, 16, 1, p(out)) == _abi.ERR_INVALID_ARGUMENT
    assert hip_lib.wax_hip_mirror_lists_probe(p(keys), 1, 16, 1, None) == _abi.ERR_INVALID_ARGUMENT


# ---- the real path ----
N, DIMS, K, GRID, N_QUERIES = 70003, 384, 10, 8, 8


def test_every_form_of_the_pass_answers_alike_on_a_store_whose_waves_prune(wax):
    rows = oracle.gaussian_unit_rows(0, N, DIMS, seed=29)
    qs = oracle.gaussian_unit_queries(N_QUERIES, DIMS, seed=31)
    eng = wax.HIPVectorEngine(metric=wax.VectorMetric(0), dimensions=DIMS)
    try:
        eng.addBatch(np.arange(N, dtype=np.uint64), rows)
        eng.setTuning("grid_blocks", GRID)
        assert eng.getTuning("scan_grid") == GRID
        eng.setTuning("scan_mirror", 0)
        eng.setTuning("mirror_share", 0)
        exact = [eng.searchArrays(q, K) for q in qs]
        eng.setTuning("mirror_bits", 8)
        eng.setTuning("scan_mirror", 2)
        for _ in range(3):                                   # the third eligible query in a row builds the code mirror
            eng.searchArrays(qs[0], K)
        assert eng.getTuning("mirror8_conversions") >= 1
        passes8, fallbacks = eng.getTuning("mirror8_passes"), eng.getTuning("mirror8_fallbacks")
        for i, q in enumerate(qs):
            keys = eng.mirror8Keys(q)
            assert len(keys) == N
            best64 = set(np.lexsort((np.arange(N), keys))[:P.KP].tolist())
            eng.setTuning("mirror_share", 0)
            answers = [("alone", eng.searchArrays(q, K))]
            eng.setTuning("mirror_share", 2)
            for g in (2, 3, 4):
                members = [(i + j) % N_QUERIES for j in range(g)]
                tickets = [eng.submit(qs[m], K) for m in members]
                got = [eng.collect(t, K) for t in tickets]
                answers.append((f"first of {g}", got[0]))
                for m, hits in zip(members[1:], got[1:]):
                    assert np.array_equal(hits[0], exact[m][0]) and np.array_equal(hits[1], exact[m][1]), f"query {m} behind query {i} in a pass of {g}"
            for name, (ids, scores) in answers:
                assert np.array_equal(ids, exact[i][0]) and np.array_equal(scores, exact[i][1]), f"query {i} {name}"
                assert set(int(x) for x in ids) <= best64, f"query {i} {name}: a returned row outside the 64 smallest keys of the pass"
        # every answer above came from a certified pass over the code mirror
        assert eng.getTuning("mirror8_fallbacks") == fallbacks and eng.getTuning("mirror8_passes") == passes8 + N_QUERIES * 4
    finally:
        eng.close()
