"""What tests/test_masked_iterations_gpu.py rests on, shown on the CPU (masked_iterations_ref.py; no engine code runs here):

  the grid rule    its stores get exactly 1, 2 and 3 workgroups under "grid_blocks" 1, 2 and 3, so a wave of the masked passes runs 22
                   to 129 iterations (up to 513 in the f32 scan at 768-d) — and the masked stores of the older files get one;
  certification    every (store, form, "grid_blocks", mask, query) on which the GPU test asserts "no fallback" certifies in the
                   float64 models of the two certificates with a margin of at least predicate_mirror_ref.MARGIN_FLOOR, at the largest
                   top_k sent (32 on bf16, 16 on 8 bits: d_k grows with k, so a smaller k has the larger margin);
  teeth            under the mask that a pass would apply if it took the word of the iteration before or behind the right one, the
                   model's best rows are other rows, for every query: such a pass cannot return the right answer by luck."""
import numpy as np
import pytest

import masked_iterations_ref as I
import predicate_mirror_ref as R

MODEL = {"bf16": I.model16, "code8": I.model8}
LARGEST_K = {"bf16": 32, "code8": 16}
TEETH_K = 10


def test_the_grid_rule_gives_the_iterations_the_masks_are_built_on():
    # 4 099 rows: 257 chunks of 16 rows, 513 of 8
    for c, per_wave in ((16, (65, 33, 22)), (8, (129, 65, 43))):
        for g, most in zip(I.GRID_BLOCKS, per_wave):
            assert I.pass_grid(I.N_SMALL, c, g) == g
            assert I.iterations(I.N_SMALL, c, 4 * g)[0] == most
    assert I.iterations(I.N_SMALL, 16, 12) == (22, 21) and I.iterations(I.N_SMALL, 8, 12) == (43, 42), "3 workgroups: a ragged last iteration"
    for dims in (384, 768):
        for g in I.GRID_BLOCKS:
            for form in I.FORMS:
                assert I.grid_of(form, I.N_SMALL, dims, g) == g, (form, dims, g)
    assert I.chunk_rows("f32", 384) == 8 and I.chunk_rows("f32", 768) == 2
    assert I.iterations(I.N_SMALL, 2, 4)[0] == 513
    # why the older masked stores run one iteration per wave: a wave per chunk at the default grid
    assert I.pass_grid(20_005, 16) == 313 and I.pass_grid(3_001, 8) == 94 and I.pass_grid(3_001, 16) == 47
    assert I.pass_grid(33, 16) == 1 and I.pass_grid(4_099, 16) == 65
    assert -(-20_005 // 16) <= 4 * 313 and -(-3_001 // 8) <= 4 * 94 and -(-4_099 // 16) <= 4 * 65
    # the store at the default grid: three iterations
    _, n, dims = I.BIG_STORE
    assert I.pass_grid(n, 16) == 342 and I.iterations(n, 16, 4 * 342) == (3, 2)
    assert I.waves_of("code8", n, dims, 0) == I.waves_of("bf16", n, dims, 0) == (16, 1368)
    # the f32 scan's own rule: the small-store branch of the default grid, the common rule under a small cap and on large stores
    assert I.scan_grid(20_011, 8) == 157 and I.scan_grid(3_001, 2) == 126 and I.scan_grid(10_000_000, 8) == 512
    assert I.scan_grid(40_000, 8) == I.pass_grid(40_000, 8) == 417


def test_masks_are_what_they_say():
    for name, (_, n, dims) in I.STORES.items():
        for form in I.FORMS:
            for g in I.GRID_BLOCKS:
                c, w = I.waves_of(form, n, dims, g)
                ms, it = I.masks_of(name, form, g), I.iteration(n, c, w)
                last = int(it[-1])
                assert last + 1 == I.iterations(n, c, w)[0]
                assert np.array_equal(ms["even"], ~ms["odd"]) and np.array_equal(ms["even"], it % 2 == 0)
                assert ms["sparse"][it == 0].all() and ms["sparse"][it == last].all() and not ms["sparse"][(it == 1) | (it == last - 1)].any()
                live = np.unique(it[ms["after_skips"]])
                assert np.array_equal(live, np.arange(7, last + 1, 8)) and len(live) >= 2
                per_chunk = np.add.reduceat(ms["one_per_chunk"].astype(int), np.arange(0, n, R.MIRROR_CHUNK[dims]))
                assert np.all(per_chunk == 1) and abs(ms["r16"].mean() - 1 / 16) < 0.01
                fl = I.flags_for(ms)
                for mask_name in I.MASKS:
                    assert np.array_equal((fl & np.uint32(I.MASK_BIT[mask_name])) == 0, ms[mask_name])
                    if form != "f32":
                        assert ms[mask_name].sum() >= 257, (name, form, g, mask_name)
                # every chunk of a wave's iteration sits in bitmap words of its own, except in the f32 scan at 768-d (shifted's docstring)
                assert ((c * w) % 32 == 0) == (not (form == "f32" and dims == 768)), (form, dims, g)


@pytest.mark.parametrize("name", list(I.STORES))
def test_every_case_held_to_no_fallback_certifies(name):
    _, n, dims = I.STORES[name]
    least = {}
    for form in ("bf16", "code8"):
        model, k = MODEL[form](name), LARGEST_K[form]
        for g in I.GRID_BLOCKS:
            for mask_name, mask in I.masks_of(name, form, g).items():
                margins = [model.margin(mask, q, k) for q in range(I.N_QUERIES)]
                key = (float(min(margins)), g, mask_name)
                least[form] = min(least.get(form, key), key)
                assert min(margins) >= R.MARGIN_FLOOR, f"{name} {form} grid_blocks {g} {mask_name} top_k {k}: margin {min(margins)}"
    # the unfiltered member of a mixed set rides the same pass over every row: certified as well
    free = [I.model8(name).margin(np.ones(n, dtype=bool), q, LARGEST_K["code8"]) for members in I.MIXED_SETS for q, m in members if m is None]
    assert len(free) == 1 and min(free) >= R.MARGIN_FLOOR, f"{name}: an unfiltered member, margin {min(free)}"
    for form, (margin, g, mask_name) in least.items():
        print(f"{name} {form}: smallest margin {margin:.4f} ({mask_name}, {g} workgroups, top_k {LARGEST_K[form]})")


def test_the_store_at_the_default_grid_certifies():
    _, n, dims = I.BIG_STORE
    for form in ("bf16", "code8"):
        model, k = MODEL[form](I.BIG), LARGEST_K[form]
        ms = I.masks_of(I.BIG, form, 0)
        margins = [model.margin(ms[mask_name], q, k) for mask_name in I.BIG_MASKS for q in range(I.BIG_QUERIES)]
        print(f"{I.BIG} {form}: smallest margin {min(margins):.4f} (top_k {k})")
        assert min(margins) >= R.MARGIN_FLOOR, (form, min(margins))
        assert ms["odd"].sum() == 16 * 1368 and ms["even"].sum() == n - 16 * 1368, "iterations 0 and 2 (ragged) against iteration 1"


@pytest.mark.parametrize("name", list(I.STORES) + [I.BIG])
def test_the_word_of_a_neighbouring_iteration_gives_other_rows(name):
    _, n, dims = I.shape_of(name)
    model = I.model16(name)                        # (its exact distances: what every form returns the best of)
    nq = len(I.queries_of(name))
    for form in I.FORMS:
        if form == "f32" and (dims == 768 or name == I.BIG):
            continue                               # 768-d: see shifted; the large store is sent through the two mirror passes only
        for g in ((0,) if name == I.BIG else I.GRID_BLOCKS):
            c, w = I.waves_of(form, n, dims, g)
            ms = I.masks_of(name, form, g)
            for mask_name in (I.BIG_MASKS if name == I.BIG else I.MASKS):
                mask = ms[mask_name]
                for by in (-1, 1):
                    wrong = I.shifted(mask, c, w, by)
                    assert wrong.sum() > 0 and not np.array_equal(wrong, mask)
                    for q in range(nq):
                        ks = (1, TEETH_K) if mask_name in ("even", "odd", "sparse", "after_skips") else (TEETH_K,)
                        for k in ks:                # (a random mask can keep its one best row under the shift: top_k 10 there)
                            right, other = I.top_ids(model, mask, q, k), I.top_ids(model, wrong, q, k)
                            assert not np.array_equal(right, other), f"{name} {form} grid_blocks {g} {mask_name} shifted by {by}: query {q} top_k {k}"
