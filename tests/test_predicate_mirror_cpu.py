"""The float64 model of the masked scan's mirror form ("predicate_mirror"), on the CPU: bf16 rounding (round to nearest
even), the mask, the 64 best approximate distances among the passing rows, the exact d_k and the finish kernel's eps written out
from mirror_finish.h (predicate_mirror_ref.py). Nothing here runs engine code.

What it establishes for tests/test_predicate_mirror_gpu.py: on every (store, mask, query, k) where that test asserts zero fallbacks
the margin a_64 - eps - d_k is above MARGIN_FLOOR, several times the f32 summation error of the kernels on both sides of the
certificate; on the store of exact duplicates the margin is negative for every query and k, so there every query falls back; and
64 or fewer passing rows never reach the form."""
import numpy as np
import pytest

import predicate_mirror_ref as R
from helpers import bf16_rne


def test_the_mirror_is_bf16_round_to_nearest_even_of_the_normalised_row():
    rows = R.store_rows("cos768")[:200]
    m, err = R.mirror_of(R.COS, rows)
    assert m.dtype == np.float32 and not np.any(m.view(np.uint32) & 0xffff), "every mirror value is a bf16"
    n = np.sqrt(np.sum(rows * rows, axis=1, dtype=np.float32))
    assert np.array_equal(m, bf16_rne((rows * (np.float32(1.0) / n)[:, None]).astype(np.float32)))
    assert np.all(np.abs(m.astype(np.float64) - rows) <= 2.0 ** -8 * np.abs(rows) + 1e-7)   # half a bf16 ulp (8 significant bits) + the normalisation
    assert 0.0 < err < 2.0 ** -8                                                 # a unit row loses less than its worst case
    d, _ = R.mirror_of(R.DOT, R.store_rows("dot768")[:200])
    assert np.array_equal(d, bf16_rne(R.store_rows("dot768")[:200]))
    z, _ = R.mirror_of(R.COS, np.zeros((2, 8), dtype=np.float32))
    assert not z.any(), "a row of norm <= 1e-6 is zeroed"


def test_eps_is_the_finish_kernels():
    """The numbers of Bf16Eps (mirror_finish.h), by hand: cosine at 768-d with a measured row error of 1.25e-3, and the unmeasured worst case."""
    e = R.finish_eps(R.COS, 768, 1.0, 1.0, 1.25e-3)
    by_hand = (1.0 + 1e-6) * float(np.float32(1.25e-3)) * 1.001 + 3.0 * 768 * 5.97e-8 * (1.0 + 1e-6) ** 2 + 3e-6
    assert by_hand <= e <= by_hand * (1 + 2.0 ** -22)
    worst = R.finish_eps(R.COS, 768, 1.0, 1.0, 0.0)
    assert abs(worst - ((0.0078125 * (1 + 1 / 512) + 768 * 5.97e-8 + 1e-6) * (1 + 1e-6) ** 2 * 1.001 + 3e-6)) < 1e-8 and worst > 3 * e
    assert R.finish_eps(R.COS, 768, 1.0, 1.0, 1.0) == worst, "a measurement above the worst case does not raise eps"
    d = R.finish_eps(R.DOT, 384, 1.5, 2.0, 2.5e-3)
    assert abs(d - (1.5 * float(np.float32(2.5e-3)) * 1.001 + 3 * 384 * 5.97e-8 * 3.0 + 1e-6 * 4.0)) < 1e-8
    for name in R.STORES:
        eps = R.model(name).eps
        assert np.all(eps > 0) and np.all(eps < 0.005), (name, eps)


def test_eps_bounds_the_models_own_approximation_error():
    """|approximate - exact| <= eps for every row and query of every store: the bound the certificate's argument rests on."""
    for name in R.STORES:
        m = R.model(name)
        assert np.all(np.abs(m.approx - m.exact) <= m.eps[None, :]), name


def test_masks_are_what_they_say():
    for name, (_, n, dims) in R.STORES.items():
        ms, c = R.masks(n, dims), R.MIRROR_CHUNK[dims]
        assert abs(ms["r15"].mean() - 15 / 16) < 0.01 and abs(ms["half"].mean() - 0.5) < 0.03
        lo, hi = R.range_bounds(n)
        assert ms["range"].sum() == hi - lo and lo % c and hi % c and (hi - lo) // c > 100, "whole chunks and waves inside and outside the range"
        if n == 20_005:
            assert hi - lo == 12_000
        per_chunk = np.add.reduceat(ms["one_per_chunk"].astype(int), np.arange(0, n, c))
        assert np.all(per_chunk == 1) and n % c, "one passing row in every chunk, the ragged last one too"
        tail = ms["tail_plus_65"]
        assert tail[n - n % c:].all() and tail.sum() == n % c + 65
        assert ms["m65"].sum() == 65 and ms["m64"].sum() == 64 and ms["m0"].sum() == 0
        fl = R.flags_for(n, dims)
        for mask_name, bit in R.MASK_BIT.items():
            assert np.array_equal((fl & np.uint32(bit)) == 0, ms[mask_name])


@pytest.mark.parametrize("name", list(R.STORES))
def test_margin_on_every_case_the_gpu_test_holds_to_zero_fallbacks(name):
    _, n, dims = R.STORES[name]
    m, ms = R.model(name), R.masks(n, dims)
    for mask_name in R.TAKEN_MASKS:
        for k in R.KS:
            margins = [m.margin(ms[mask_name], q, k) for q in range(R.N_QUERIES)]
            assert min(margins) > R.MARGIN_FLOOR, (name, mask_name, k, min(margins))


def test_margins_of_the_unit_row_store_are_the_designs():
    """The figures DESIGN 4.5 quotes for 20 005 unit rows at 384-d, top_k 10 and 32 (minimum over the 16 queries)."""
    m, ms = R.model("cos384"), R.masks(20_005, 384)
    least = lambda mask, k: min(m.margin(ms[mask], q, k) for q in range(R.N_QUERIES))   # noqa: E731
    assert 0.015 < least("r15", 10) < 0.03 and 0.015 < least("half", 10) < 0.03 and 0.015 < least("range", 10) < 0.03
    assert 0.004 < least("r15", 32) < 0.01 and 0.004 < least("half", 32) < 0.01 and 0.004 < least("range", 32) < 0.01
    assert least("m65", 10) > 0.08
    assert abs(m.eps[0] - 0.0021) < 2e-4


def test_a_store_of_exact_duplicates_never_certifies():
    """70 passing copies of every distinct row: the 64 best approximate distances are all the best row's, so a_64 - d_k <= a_1 - d_1 <= the
    rounding error < eps for every k."""
    m, mask = R.dup_model(), R.dup_mask()
    assert mask.sum() == R.DUP_PASSING > R.MIRROR_KP
    assert np.array_equal(R.dup_rows()[:256], R.dup_rows()[256:512])
    for q in range(R.N_QUERIES):
        for k in R.KS:
            assert m.margin(mask, q, k) < -1e-3, (q, k)


def test_64_or_fewer_passing_rows_never_reach_the_form():
    for name, (metric, n, dims) in R.STORES.items():
        m, ms = R.model(name), R.masks(n, dims)
        for mask_name in R.NOT_TAKEN_MASKS:
            assert m.margin(ms[mask_name], 0, 1) == -np.inf
            assert not R.takes_mirror_form(metric, dims, 1, int(ms[mask_name].sum()))
        assert R.takes_mirror_form(metric, dims, 32, 65) and not R.takes_mirror_form(metric, dims, 33, 10_000)
        assert not R.takes_mirror_form(metric, dims, 10, 64) and not R.takes_mirror_form(metric, dims, 10, 10_000, mode=0)
    assert not R.takes_mirror_form(2, 384, 10, 10_000) and not R.takes_mirror_form(R.COS, 100, 10, 10_000)
