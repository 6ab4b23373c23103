"""tests/pass_lists_ref.py, the host model that tests/test_pass_lists_gpu.py holds the selection frame to, against a brute-force walk:
every slot to its wave and workgroup one by one, a plain sort per workgroup."""
import numpy as np

import pass_lists_ref as P


def brute(keys, grid):
    nq, n_slots = keys.shape
    offered = [[[] for _ in range(grid)] for _ in range(nq)]
    nwaves = P.WAVES * grid
    for slot in range(n_slots):
        chunk = slot // P.TILE
        gwave = chunk % nwaves                    # wave g takes chunks g, g + nwaves, ...
        for q in range(nq):
            if keys[q, slot] != P.PAD:
                offered[q][gwave // P.WAVES].append(int(keys[q, slot]))
    out = np.full((nq, grid, P.KP), P.PAD, dtype=np.int64)
    for q in range(nq):
        for b in range(grid):
            best = sorted(offered[q][b])[:P.KP]
            out[q, b, :len(best)] = best
    return out


def test_the_model_is_a_sort_per_workgroup():
    rng = np.random.default_rng(3)
    for grid, n_slots in ((1, 5), (1, 700), (2, 2049), (3, 4000), (8, 3001)):
        keys = P.make_key(rng.integers(-(1 << 30), 1 << 30, size=(3, n_slots)), np.arange(n_slots))
        keys[1, rng.random(n_slots) < 0.7] = P.PAD
        keys[2, : n_slots // 2] = P.PAD
        assert np.array_equal(P.partials(keys, grid), brute(keys, grid)), (grid, n_slots)


def test_keys_order_like_the_scan():
    assert P.make_key(P.NEG_INF_WORD, 7) < P.make_key(-5, 0) < P.make_key(-5, 1) < P.make_key(0, 0) < P.make_key(1 << 30, 0) < P.PAD
    assert int(P.make_key(3, 9)) == (3 << 32) | 9


def test_streams_land_in_their_waves():
    grid = 2
    streams = [list(P.make_key(np.full(20 + w, w), np.arange(20 + w))) for w in range(P.WAVES * grid)]
    keys = P.from_streams(streams, grid)
    assert len(keys) == 2 * P.TILE * P.WAVES * grid
    wg = P.workgroup_of_slots(len(keys), grid)
    for slot, key in enumerate(keys):
        if key != P.PAD:
            w = int(key >> 32)
            assert (slot // P.TILE) % (P.WAVES * grid) == w and wg[slot] == w // P.WAVES
    for w, s in enumerate(streams):
        mine = keys.reshape(-1, P.WAVES * grid, P.TILE)[:, w, :].reshape(-1)
        assert list(mine[:len(s)]) == [int(x) for x in s] and np.all(mine[len(s):] == P.PAD)
