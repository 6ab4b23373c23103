"""The constructions behind tests/test_mirror_edges_gpu.py, proved on the CPU in f64: the generators in helpers.py build what they
say, and each one really reaches the edge it is aimed at. Nothing here runs engine code: the arithmetic is numpy's and the oracle's."""
import numpy as np

import oracle
from helpers import (ANTI_GAP, ANTI_SPREAD, ANTI_TOP, ANTI_TOP_STEP, THRESHOLD, THRESHOLD_COS_STEP, THRESHOLD_TOP_COS,
                     anti_correlated_corpus, bf16_rne, f32_norm2_chain_order, f32_norm2_scan_order, threshold_rows)

ANTI_SEED = 101          # the seeds the GPU tests use
THRESHOLD_SEED = 202


def f32(bits):
    return np.array([bits], dtype=np.uint32).view(np.float32)[0]


def bits(x):
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0])


def test_bf16_rne_hand_cases():
    cases = [
        (0x3f800000, 0x3f800000),   # 1.0
        (0x3f808000, 0x3f800000),   # midpoint above an even mantissa: down
        (0x3f818000, 0x3f820000),   # midpoint above an odd mantissa: up
        (0x3f808001, 0x3f810000),   # just above a midpoint
        (0x3f807fff, 0x3f800000),   # just below a midpoint
        (0xbf818000, 0xbf820000),   # the sign does not matter
        (0x7f7fffff, 0x7f800000),   # the largest finite f32 -> inf
        (0x7f7f8000, 0x7f800000),   # the midpoint between the largest bf16 and inf: ties to even = inf
        (0x7f7f7fff, 0x7f7f0000),   # just below it: the largest bf16 (3.3895e38)
        (0x7f800000, 0x7f800000),   # inf
        (0xff800000, 0xff800000),   # -inf
        (0x00000001, 0x00000000),   # the smallest denormal -> 0
        (0x00008000, 0x00000000),   # denormal midpoint above an even mantissa (0)
        (0x00018000, 0x00020000),   # denormal midpoint above an odd mantissa
        (0x007fffff, 0x00800000),   # the largest denormal -> the smallest normal
        (0x80000000, 0x80000000),   # -0
    ]
    for src, want in cases:
        got = bits(bf16_rne(np.array([f32(src)], dtype=np.float32))[0])
        assert got == want, (hex(src), hex(got), hex(want))
    for nan_bits in (0x7fc00000, 0x7f800001, 0xffc12345):
        assert np.isnan(bf16_rne(np.array([f32(nan_bits)], dtype=np.float32))[0])
    assert np.isinf(bf16_rne(np.array([3.4e38], dtype=np.float32))[0])
    assert bf16_rne(np.array([3.389e38], dtype=np.float32))[0] == np.float32(3.3895314e38)
    assert bf16_rne(np.zeros((3, 5), dtype=np.float32)).shape == (3, 5)


def test_bf16_rne_equals_torch():
    import torch
    rng = np.random.default_rng(0)
    x = rng.standard_normal(200_000).astype(np.float32) * np.exp2(rng.integers(-140, 127, 200_000)).astype(np.float32)
    raw = rng.integers(0, 2 ** 32, 200_000, dtype=np.uint64).astype(np.uint32).view(np.float32)   # every bit pattern, NaN and inf included
    for arr in (x, raw):
        want = torch.from_numpy(arr.copy()).bfloat16().float().numpy()
        got = bf16_rne(arr)
        both_nan = np.isnan(got) & np.isnan(want)
        assert np.array_equal(got.view(np.uint32)[~both_nan], want.view(np.uint32)[~both_nan])
        assert np.array_equal(np.isnan(got), np.isnan(want))


def cosines64(rows, q):
    r, q = rows.astype(np.float64), q.astype(np.float64)
    return (r @ q) / (np.linalg.norm(r, axis=1) * np.linalg.norm(q))


def test_anti_correlated_corpus_is_what_it_says():
    for dims, zero_at in ((384, None), (384, 17), (768, 17)):
        rows, q = anti_correlated_corpus(20000, dims, ANTI_SEED, zero_at=zero_at)
        assert zero_at is None or q[zero_at] == 0.0
        assert rows.dtype == np.float32 and rows.shape == (20000, dims) and q.dtype == np.float32
        assert np.max(np.abs(np.linalg.norm(rows.astype(np.float64), axis=1) - 1.0)) < 1e-6
        assert abs(np.linalg.norm(q.astype(np.float64)) - 1.0) < 1e-6
        c = np.sort(cosines64(rows, q))[::-1]
        assert c[0] <= -0.05 and c[0] > -0.0501
        # f32 rows: every element carries 2^-24 relative, a cosine of unit vectors <= 2 * 2^-24 ~ 1.2e-7 absolute; 1e-6 is generous
        assert np.max(np.abs(np.diff(c[:ANTI_TOP]) + ANTI_TOP_STEP)) < 1e-6
        assert c[ANTI_TOP - 1] - c[ANTI_TOP] >= ANTI_GAP - 1e-6
        assert c[-1] >= c[ANTI_TOP - 1] - ANTI_GAP - ANTI_SPREAD - 1e-6
        assert np.argmax(cosines64(rows, q)) > 100      # shuffled: the best rows are not the first rows


def test_anti_correlated_corpus_leaves_the_certificate_no_honest_reason_to_refuse():
    """In f64 over the bf16 rounding of the (f32-normalised) rows: the 64th smallest approximate distance exceeds the 32nd smallest
    exact distance by more than 0.02, five times the eps ~ 0.0037 of DESIGN 4.4 — for every k <= 32."""
    for dims in (384, 768):
        rows, q = anti_correlated_corpus(20000, dims, ANTI_SEED, zero_at=17)
        exact = 1.0 - cosines64(rows, q)
        unit = (rows / np.sqrt(np.sum(rows * rows, axis=1, dtype=np.float32))[:, None]).astype(np.float32)
        approx = 1.0 - (bf16_rne(unit).astype(np.float64) @ q.astype(np.float64)) / np.linalg.norm(q.astype(np.float64))
        assert np.max(np.abs(approx - exact)) < 0.0037
        assert np.sort(approx)[63] - np.sort(exact)[31] > 0.02


def test_planted_special_rows_score_zero_and_rank_first_in_the_oracle():
    """What the GPU test expects of the cosine metric, checked on the oracle alone: a NaN row, a zero row and a row of norm 1e-7
    score exactly 0.0 and come before every ordinary row of the anti-correlated corpus."""
    dims = 384
    rows, q = anti_correlated_corpus(2000, dims, ANTI_SEED)
    rows[3, 7] = np.nan
    rows[900] = 0.0
    rows[1990] *= np.float32(1e-7)
    ids, scores, _, _ = oracle.search(0, rows, None, q, 10)
    assert sorted(ids[:3].tolist()) == [3, 900, 1990] and np.all(scores[:3] == 0.0)
    assert np.all(scores[3:] <= -0.05 + 1e-6)


def test_threshold_rows_norms_and_cosines():
    for dims in (384, 768):
        q = oracle.gaussian_unit_queries(1, dims)[0]
        rows, c, j = threshold_rows(q, 256, dims, THRESHOLD_SEED)
        assert rows.dtype == np.float32 and rows.shape == (256, dims)
        assert j.min() == -32 and j.max() == 32 and len(set(j.tolist())) == 65
        assert c[0] == THRESHOLD_TOP_COS and abs(c[255] - 0.700) < 1e-12 and np.allclose(np.diff(c), -THRESHOLD_COS_STEP, atol=1e-12)
        assert abs((c[31] - c[63]) - 0.032) < 1e-12
        # the f32 cast moves every element by <= 2^-24 relative, hence the norm by <= 2^-24 relative: one step of j
        norms = np.linalg.norm(rows.astype(np.float64), axis=1)
        assert np.max(np.abs(norms / 1e-6 - (1.0 + j * 2.0 ** -24))) <= 2.0 ** -24
        assert np.max(np.abs(cosines64(rows, q) - c)) < 1e-6
        assert np.min(np.abs(rows[rows != 0])) > 1e-30          # no denormal squares: the f32 sums see every element


def test_threshold_rows_straddle_the_rule_under_two_f32_summation_orders():
    """Two honest f32 ways of summing the same squares — one accumulator per lane over 64 lanes, and the f32 scan's four
    accumulators per lane over 32 (384-d) / 64 (768-d) lanes — put at least one constructed row on opposite sides of
    `sqrt(m) > 1e-6f`; and on each side of the rule there are rows both orders agree on."""
    for dims, group in ((384, 32), (768, 64)):
        q = oracle.gaussian_unit_queries(1, dims)[0]
        rows, _, j = threshold_rows(q, 256, dims, THRESHOLD_SEED)
        chain = np.sqrt(f32_norm2_chain_order(rows)) > THRESHOLD
        scan = np.sqrt(f32_norm2_scan_order(rows, group)) > THRESHOLD
        assert chain.dtype == bool and np.sqrt(f32_norm2_chain_order(rows)).dtype == np.float32
        assert np.count_nonzero(chain != scan) >= 1, (dims, "no row straddles: pick another THRESHOLD_SEED")
        assert np.all(chain[j >= 8]) and np.all(scan[j >= 8]) and not np.any(chain[j <= -8]) and not np.any(scan[j <= -8])
        # both are sums of the same numbers: they agree with the f64 sum to a few ulp
        m64 = np.sum(rows.astype(np.float64) ** 2, axis=1)
        assert np.max(np.abs(f32_norm2_chain_order(rows) / m64 - 1.0)) < 8 * 2.0 ** -24
        assert np.max(np.abs(f32_norm2_scan_order(rows, group) / m64 - 1.0)) < 8 * 2.0 ** -24


def test_adversarial_variants_lose_what_they_say():
    """bf16_adversarial_unit_vector(dims, frac): a unit vector whose rounding error norm is frac * 2^-8 (of norm 1), so a row of a
    larger frac raises the store's true maximum."""
    from helpers import bf16_adversarial_unit_vector
    last = 0.0
    for frac in (0.90, 0.92, 0.94, 0.96, 0.97, 0.98, 0.99):
        x = bf16_adversarial_unit_vector(384, frac, roll=5)
        assert abs(np.linalg.norm(x.astype(np.float64)) - 1.0) < 1e-6 and x[4] == 0 and x[5] != 0
        err = np.linalg.norm(x.astype(np.float64) - bf16_rne(x).astype(np.float64))
        assert abs(err / (frac * 2.0 ** -8 / (1 + frac * 2.0 ** -8)) - 1.0) < 1e-3 and err > last
        last = err
    assert np.array_equal(bf16_adversarial_unit_vector(384), bf16_adversarial_unit_vector(384, 0.99, 0))
