"""Host model of the selection frame of a mirror pass (mirror_pass.h: PassLists) as wax_hip_mirror_lists_probe runs it: what every
workgroup keeps for every query, whatever its waves did on the way (prunes, the workgroup's bound, joint or single).

The walk is the pass's: slots in tiles of 16, tile c to wave c mod (4 * grid) of the launch, wave g in workgroup g // 4. A workgroup's
partials for a query are the 64 smallest keys it was offered for that query, ascending, PAD behind them; PAD in the input marks a slot
that is not offered. Keys are (ordered distance word : row) like the scan's, so no key occurs twice."""
import numpy as np

KP, CAP, TILE, WAVES = 64, 128, 16, 4
PAD = (1 << 63) - 1
NEG_INF_WORD = -2139095041        # order_bits(-inf): the word of a row that is always a candidate


def make_key(word, row):
    """(word : row) as the scan packs it; word is a signed 32-bit ordered distance"""
    return (np.asarray(word, dtype=np.int64) << 32) | np.asarray(row, dtype=np.int64)


def workgroup_of_slots(n_slots, grid):
    """[n_slots] the workgroup whose wave walks each slot"""
    return ((np.arange(n_slots) // TILE) % (WAVES * grid)) // WAVES


def partials(keys, grid):
    """keys: [nq][n_slots] int64 -> [nq][grid][KP] int64"""
    keys = np.asarray(keys, dtype=np.int64)
    nq, n_slots = keys.shape
    wg = workgroup_of_slots(n_slots, grid)
    out = np.full((nq, grid, KP), PAD, dtype=np.int64)
    for q in range(nq):
        for b in range(grid):
            mine = keys[q][wg == b]
            best = np.sort(mine[mine != PAD])[:KP]
            out[q, b, :len(best)] = best
    return out


def from_streams(streams, grid):
    """streams[w]: the keys wave w of the launch (0 .. 4 * grid - 1) meets, in the order of its walk (PAD = a hole); a stream is padded
    with holes to whole tiles and the shorter streams to the longest -> [n_slots] int64"""
    nwaves = WAVES * grid
    assert len(streams) == nwaves
    tiles = max(1, max((len(s) + TILE - 1) // TILE for s in streams))
    out = np.full((tiles, nwaves, TILE), PAD, dtype=np.int64)
    for w, s in enumerate(streams):
        s = np.asarray(s, dtype=np.int64)
        flat = np.full(tiles * TILE, PAD, dtype=np.int64)
        flat[:len(s)] = s
        out[:, w, :] = flat.reshape(tiles, TILE)
    return out.reshape(-1)
