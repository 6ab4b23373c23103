"""The stores, the masks and the grid rule behind tests/test_masked_iterations_cpu.py and tests/test_masked_iterations_gpu.py.

Three kernels scan the store under a row bitmap in a persistent grid: code8_pass<MASKED> (mirror8_scan.hip, the predicate tickets'
pass over the 8-bit code mirror), mirror_pass<MASKED> (mirror_pass.h, the bf16 mirror form of a predicate search) and
scan_masked_kernel (predicate.hip, the f32 store). Wave w of W = 4 * grid owns chunks w, w + W, w + 2 W, ... of C rows each; it
fetches the bitmap word of its next chunk one iteration ahead, takes this iteration's bits from the word fetched in the previous one,
and leaves a chunk without a passing row before anything else is done. The masks here are built on the ITERATION it(row) =
(row // C) // W that owns a row, so that the word of a neighbouring iteration is never the right one, and the stores are small
enough for "grid_blocks" 1, 2 and 3 to give a wave 22 to 129 iterations.

The grid rule is restated below (pass_grid, scan_grid). No answer depends on it: the GPU test holds every answer to references that
know nothing of iterations. Only the masks' power to catch a wrong word does, and the CPU test pins the values used."""
import functools

import numpy as np

import oracle
import predicate_mirror_ref as R

COS, DOT = R.COS, R.DOT
SCAN_WAVES = 4                       # waves per scan workgroup (common.h)
PASS_GRID_MAX = 512                  # SCAN_KWAY_MERGE_GRID: the most workgroups a mirror pass is given
SCAN_GRID_MAX = 8192                 # MAX_GRID_BLOCKS
SCAN_FUSE_MERGE_GRID = 160           # the small-store rule of the f32 scan keeps the grid at or below this
CODE8_CHUNK = {384: 16, 768: 16}     # a 16-row tile per wave iteration of the 8-bit pass

STORE_SEED, QUERY_SEED, N_QUERIES = 20261020, 23, 8
N_SMALL = 4_099
# name -> (metric, rows, dims)
STORES = {"cos384": (COS, N_SMALL, 384), "cos768": (COS, N_SMALL, 768), "dot384": (DOT, N_SMALL, 384), "dot768": (DOT, N_SMALL, 768)}
GRID_BLOCKS = (1, 2, 3)
FORMS = ("code8", "bf16", "f32")
KS = {"code8": (1, 10, 16), "bf16": (1, 10, 16, 32), "f32": (1, 10, 16, 100)}
MASKS = ("even", "odd", "sparse", "after_skips", "r16", "one_per_chunk")
MASK_BIT = {name: 1 << (8 + i) for i, name in enumerate(MASKS)}

# the store at the default grid: 65 553 x 384, cosine, 4 queries, the masks even / odd
BIG = "big384"
BIG_STORE = (COS, 65_553, 384)
BIG_QUERIES = 4
BIG_MASKS = ("even", "odd")

# the 8-bit sets whose members carry different masks: (query, mask; None = an unfiltered ticket)
MIXED_SETS = ([(0, "even"), (1, "odd")],                                  # no tile is skipped; each member only its own rows
              [(2, "sparse"), (3, "after_skips")],                        # a tile is skipped only where both are dead
              [(4, "even"), (5, "odd"), (6, "sparse"), (7, None)],        # the null bitmap keeps every tile live
              [(0, "r16"), (1, "one_per_chunk"), (2, "after_skips")])     # three members: the fourth column group is dead lanes
BIG_MIXED_SETS = ([(0, "even"), (1, "odd"), (2, "odd"), (3, "even")],)


# ---- the grid rule -------------------------------------------------------------------------------------------------------------------

def pass_grid(n, rows_per_chunk, grid_blocks=0):
    """mirror_pass_grid (mirror_pass.h): a wave per chunk up to 4 x grid_blocks (default 512) waves, beyond that every wave the same
    number of iterations."""
    cap = 512 if grid_blocks <= 0 else min(grid_blocks, PASS_GRID_MAX)
    nchunks = -(-n // rows_per_chunk)
    max_waves = cap * SCAN_WAVES
    waves = nchunks
    if nchunks > max_waves:
        iters = -(-nchunks // max_waves)
        waves = -(-nchunks // iters)
    return max(1, min(-(-waves // SCAN_WAVES), cap))


def scan_grid(n, rows_per_chunk, grid_blocks=0):
    """scan_grid_for (kernels.hip) at variant 0, which launch_scan_masked calls with scan_masked_chunk_rows: mirror_pass_grid's rule,
    and 64 .. 2 560 chunks under a cap of at least 160 workgroups share out over at most 640 waves."""
    cap = 512 if grid_blocks <= 0 else min(grid_blocks, SCAN_GRID_MAX)
    nchunks = -(-n // rows_per_chunk)
    max_waves, small_waves = cap * SCAN_WAVES, SCAN_FUSE_MERGE_GRID * SCAN_WAVES
    waves = nchunks
    if 64 <= nchunks <= 4 * small_waves and cap >= SCAN_FUSE_MERGE_GRID:
        iters = -(-nchunks // small_waves)
        waves = -(-nchunks // iters)
    elif nchunks > max_waves:
        iters = -(-nchunks // max_waves)
        waves = -(-nchunks // iters)
    return max(1, min(-(-waves // SCAN_WAVES), cap))


def chunk_rows(form, dims):
    """C: the rows of one wave iteration of the form."""
    return {"code8": CODE8_CHUNK, "bf16": R.MIRROR_CHUNK, "f32": R.F32_CHUNK}[form][dims]


def grid_of(form, n, dims, grid_blocks):
    return (scan_grid if form == "f32" else pass_grid)(n, chunk_rows(form, dims), grid_blocks)


def waves_of(form, n, dims, grid_blocks):
    """(C, W) of a pass of the form over n rows under "grid_blocks"."""
    return chunk_rows(form, dims), SCAN_WAVES * grid_of(form, n, dims, grid_blocks)


def iteration(n, c, w):
    """it(row): the wave iteration that owns the row."""
    return (np.arange(n) // c) // w


def iterations(n, c, w):
    """(the most, the fewest) iterations a wave that has a chunk at all runs."""
    nchunks = -(-n // c)
    return -(-nchunks // w), max(1, nchunks // w)


# ---- stores --------------------------------------------------------------------------------------------------------------------------

def shape_of(name):
    return BIG_STORE if name == BIG else STORES[name]


@functools.lru_cache(maxsize=None)
def store_rows(name):
    """predicate_mirror_ref.store_rows's recipe with this file's seed: Gaussian unit rows, norms 0.5 .. 2 for dot."""
    metric, n, dims = shape_of(name)
    x = oracle.gaussian_unit_rows(0, n, dims, seed=STORE_SEED + (1 if name == BIG else 0))
    if metric == DOT:
        x = x * np.random.default_rng(STORE_SEED + 7).uniform(0.5, 2.0, size=(n, 1)).astype(np.float32)
    x = np.ascontiguousarray(x, dtype=np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def queries(dims, count=N_QUERIES):
    q = oracle.gaussian_unit_queries(count, dims, seed=QUERY_SEED)
    q.setflags(write=False)
    return q


def queries_of(name):
    _, _, dims = shape_of(name)
    return queries(dims, BIG_QUERIES if name == BIG else N_QUERIES)


# ---- masks ---------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def masks(n, dims, c, w):
    """name -> the rows that pass (bool[n]) for a pass of C = c rows per iteration on W = w waves.
      even, odd       it % 2: the word of either neighbouring iteration is the complement
      sparse          it == 0 (the word fetched in front of the loop), it == last (the one behind the final `next < nchunks`) and
                      it % 16 == 5: long runs of skipped chunks between live ones
      after_skips     it % 8 == 7: seven skipped chunks, then a live one
      r16             each row passes with probability 1 / 16
      one_per_chunk   predicate_mirror_ref.masks's: one row of every bf16 chunk (16 rows at 384-d, 8 at 768-d)
    The last two do not depend on W: neighbouring words differ in almost every bit."""
    it = iteration(n, c, w)
    last = int(it[-1])
    rng = np.random.default_rng(STORE_SEED + 1)
    out = {"even": it % 2 == 0, "odd": it % 2 == 1,
           "sparse": (it == 0) | (it == last) | (it % 16 == 5),
           "after_skips": it % 8 == 7,
           "r16": rng.random(n) < 1.0 / 16.0}
    cm = R.MIRROR_CHUNK[dims]
    one = np.zeros(n, dtype=bool)
    for first in range(0, n, cm):
        one[first + rng.integers(0, min(cm, n - first))] = True
    out["one_per_chunk"] = one
    for v in out.values():
        v.setflags(write=False)
    return out


def masks_of(name, form, grid_blocks):
    _, n, dims = shape_of(name)
    return masks(n, dims, *waves_of(form, n, dims, grid_blocks))


def flags_for(ms):
    """The flag column that carries the masks `ms` (name -> bool[n]): a row FAILS mask `name` iff MASK_BIT[name] is set."""
    fl = np.zeros(len(next(iter(ms.values()))), dtype=np.uint32)
    for name, m in ms.items():
        fl[~m] |= np.uint32(MASK_BIT[name])
    return fl


def shifted(mask, c, w, by):
    """The mask a pass would apply if every wave took its bits from the word of iteration it + by: row r is judged by the bit of row
    r + by * c * w, the same position of the chunk that the wave owns `by` iterations later (no row there: no bit). In every form
    but the f32 scan at 768-d, c * w is a multiple of 32: the two rows sit at the same place of different bitmap words, which is what
    the kernels' shift by (row & 31) would make of the wrong word. At 768-d the f32 scan's neighbouring iterations lie 8, 16 or 24
    rows apart (2 rows x 4, 8 or 12 waves) and share a bitmap word three times, twice or once out of four: there the word of the wrong
    iteration is often the right word, this function overstates what such a pass would get wrong, and the CPU test proves nothing
    with it for that form (a refresh that is lost altogether leaves the first word in place and shows at once)."""
    n = len(mask)
    src = np.arange(n) + by * c * w
    ok = (src >= 0) & (src < n)
    out = np.zeros(n, dtype=bool)
    out[ok] = mask[src[ok]]
    return out


# ---- the float64 models --------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def model16(name):
    """The bf16 certificate's model (predicate_mirror_ref.Model) of a store of this file."""
    metric, _, _ = shape_of(name)
    return R.Model(metric, store_rows(name), queries_of(name))


@functools.lru_cache(maxsize=None)
def model8(name):
    """The masked 8-bit certificate's model (mirror8_ref.MaskedModel) of a store of this file."""
    import mirror8_ref as M8
    metric, _, _ = shape_of(name)
    return M8.MaskedModel(metric, store_rows(name), queries_of(name))


def top_ids(model, mask, q, k):
    """The rows of the model's k best exact distances among the passing rows, (distance, row) ascending."""
    rows = np.flatnonzero(mask)
    order = np.lexsort((rows, model.exact[rows, q]))
    return rows[order[:k]]
