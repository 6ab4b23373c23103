"""The wide mirror finish in numpy: the selection's definition, the certificate in float64. No engine code runs here."""
import numpy as np

import mirror8_ref as R

KP, PAD = 64, np.iinfo(np.int64).max
ALL, TAIL, RANK = 0, 1, 2
KS = (33, 64, 65, 256, 257, 1000, 1024)
# (rows, dims, metric, "grid_blocks"): 1 and 3 lists, the default grid, and 63 lists of ~317 rows (T cuts inside the candidates)
STORES = [(257, 384, 0, 1), (257, 384, 1, 3), (4097, 384, 0, 3), (4097, 384, 1, 1), (4097, 768, 0, 3), (4097, 768, 1, 512),
          (20005, 384, 0, 512), (20005, 384, 1, 512), (20005, 384, 0, 64)]


def keys_of(dist, rows):
    """make_key (common.h): the ordered bits of the f32 distance over the row."""
    b = np.asarray(dist, dtype=np.float32).view(np.int32).astype(np.int64)
    return ((b ^ ((b >> 31) & 0x7FFFFFFF)) << 32) | np.asarray(rows, dtype=np.int64)


def select_model(lists, c):
    """The definition in include/wax_hip.h (wax_hip_mirror_wide_probe): -> (sorted candidates, B, source)."""
    lists = np.asarray(lists, dtype=np.int64)
    live = np.sort(lists[lists != PAD])
    tails = lists[:, KP - 1]
    t = int(tails[tails != PAD].min()) if np.any(tails != PAD) else PAD
    k_c = int(live[c]) if len(live) > c else PAD
    b = min(t, k_c)
    return live[live < b], b, ALL if b == PAD else (TAIL if t <= k_c else RANK)


GUARD = 1e-4    # the device's keys are f32 sums, within D 2^-24 ||q|| ||v|| + a few ulps < 3e-5 of these on either side of the inequality


def f64_margins(x, metric, q, bits, ks, ms):
    """Per (k, m): dist(B) - eps - d_k when the m best approximate keys are the candidates (every other row has a key >= B, so B has
    rank m); +inf where every row is one. eps is Mirror8Slack, or Bf16Eps at its worst case (never below the device's)."""
    n, dims = x.shape
    qn, vmax = float(np.linalg.norm(q.astype(np.float64))), float(np.max(np.linalg.norm(x.astype(np.float64), axis=1)))
    xhat = R.normalise(x, metric)
    if bits == 8:
        approx, eps = R.lower_bounds(q, *R.quantise(xhat), metric), R.slack(dims, metric, qn, vmax)
    else:
        u = xhat.view(np.uint32).astype(np.uint64)                                   # bf16, ties to even
        s = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32).astype(np.float64) @ q.astype(np.float64)
        both = (1.0 + 1e-6) ** 2 if metric == 0 else qn * vmax
        approx = 1.0 - s / qn if metric == 0 else 1.0 - s
        eps = (0.0078125 * (1 + 1 / 512) + dims * 5.97e-8 + 1e-6) * both * 1.001 + (3e-6 if metric == 0 else 1e-6 * (1 + both))
    order = np.lexsort((np.arange(n), approx))
    exact = R.exact_distances(x, q, metric)[order]
    return [np.inf if m >= n else -np.inf if m < min(k, n) else float(approx[order[m]] - eps - np.sort(exact[:m])[min(k, n) - 1])
            for k, m in zip(ks, ms)]
