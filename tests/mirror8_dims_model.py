"""A float64 model of the certificate of searchMirror(bits=8) ("The code mirror at 512, 1 024 and 1 536 dimensions"), for
choosing the candidate count and the inputs of tests/test_mirror8_dims_gpu.py. Run it to print the margins that file quotes.

A row x^ (unit norm) is coded as code = rint(x^ / scale), scale = max|x^| / 127, err = ||scale code - x^||; its key for query q is
lb = 1 - q.(scale code) / ||q|| - err, a lower bound of d = 1 - q.x^ / ||q||. A pass leaves one list of the 64 smallest keys per
workgroup (64 consecutive rows each at these sizes), the selection takes the C smallest listed keys under B = min(T, K_C) — T the
smallest last key of a full list, K_C the listed key of rank C — and the query certifies iff dist(B) - slack > d_k."""
import numpy as np


def slack(dims):                                   # Mirror8Slack, cosine
    u = 5.97e-8
    return (8192.0 * u * np.sqrt(dims) / 127.0 + 3.0 * dims * u) * (1 + 1e-6) ** 2 * 1.001 + 3e-6


def margins(corpus, queries, k, c, rows=None):
    """dist(B) - slack - d_k per query (inf: every row that may be offered is re-scored); `rows`: the rows that pass a mask"""
    v, q = corpus.astype(np.float64), queries.astype(np.float64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    scale = np.abs(v).max(axis=1, keepdims=True) / 127.0
    coded = np.rint(v / scale) * scale
    err = np.linalg.norm(coded - v, axis=1)
    qn = q / np.linalg.norm(q, axis=1, keepdims=True)
    lb, d = 1.0 - coded @ qn.T - err[:, None], 1.0 - v @ qn.T
    keep = np.zeros(len(v), bool)
    keep[np.arange(len(v)) if rows is None else rows] = True
    out = []
    for j in range(len(q)):
        lists = [np.sort(lb[b:b + 64, j][keep[b:b + 64]]) for b in range(0, len(v), 64)]
        tails = [l[63] for l in lists if len(l) == 64]
        listed = np.sort(np.concatenate(lists))
        bound = min(tails + ([listed[c]] if len(listed) > c else []), default=np.inf)
        out.append(bound - slack(v.shape[1]) - np.sort(d[keep, j])[k - 1])
    return np.array(out)


if __name__ == "__main__":
    SEED = {512: 12, 1024: 11, 1536: 88}                   # test_mirror8_dims_gpu.py's inputs

    def unit_rows(n, dims, seed):
        v = np.random.default_rng(seed).standard_normal((n, dims))
        return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)

    for dims in (512, 1024, 1536):
        for n in (257, 4097, 9999):
            corpus, queries = unit_rows(n, dims, 1000 * SEED[dims] + dims + n), unit_rows(9, dims, 1000 * SEED[dims] + dims)
            print(dims, n, "slack %.2e" % slack(dims), {c: round(float(margins(corpus, queries, 16, c).min()), 4) for c in (64, 128, 256, 512, 1024)})
    for dims, n in ((512, 9999), (1024, 4097), (1536, 4097)):          # the masked cases: five queries, k = 10
        corpus, queries = unit_rows(n, dims, 1000 * SEED[dims] + dims + n), unit_rows(9, dims, 1000 * SEED[dims] + dims)[:5]
        for name, rows in (("a random half", np.flatnonzero(np.random.default_rng(n).random(n) >= 0.5)), ("rows 1 000 .. 1 255", np.arange(1000, 1256))):
            print(dims, n, name, "k = 10, 128 candidates:", round(float(margins(corpus, queries, 10, 128, rows).min()), 4))
