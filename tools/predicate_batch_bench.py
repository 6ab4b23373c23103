#!/usr/bin/env python3
"""wax_hip_search_batch_predicate against the two things a caller could do before it ("Batched predicates").

Store: --rows x 384 cosine (default 1M), --queries queries (default 256), top-10, timestamps ascending with the row, one status bit on
a random 1/16 of the rows. Three cases:
  (i)   one contiguous window of 1/16 of the rows for all queries;
  (ii)  16 distinct windows of 1/16, 16 queries each;
  (iii) denyFlags = 0b111, the default FrameFilter().
Three forms per case, blocking calls, alternated on one box, medians of --reps:
  (a) the loop of wax_hip_search_predicate (searchFiltered with timeRange / denyFlags);
  (b) wax_hip_search_batch_filtered with the passing ids built on the host from the host's own copy of the columns and passed as
      allow-lists, the host time included;
  (c) the new call.
(a) and (b) are what the parent commit offers; the figure per case is c against the better of them. Before timing, (c)'s rows are
checked against (a)'s, bit for bit. Prints one JSON line and, with --out, writes the same object to a file."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import torch  # noqa: E402
import wax_amd as wax  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--queries", type=int, default=256)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--out", default=None)
args = ap.parse_args()

torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
rows, dims, k, nq = args.rows, 384, 10, args.queries
eng = wax.HIPVectorEngine(dimensions=dims)
eng.reserve(rows)
for r0, x in bench.device_rows(torch, 0, rows, dims, dev):
    eng.addBatchDevice(np.arange(r0, r0 + x.shape[0], dtype=np.uint64), x)
ids = np.arange(rows, dtype=np.uint64)
ts = ids.astype(np.int64)
rng = np.random.default_rng(0)
flags = np.zeros(rows, dtype=np.uint32)
flags[rng.random(rows) < 1 / 16] = 1
eng.setAttributes(ids, ts, flags)
queries = np.ascontiguousarray(bench.unit_queries(nq, dims), dtype=np.float32)
span = rows // 16


def window(j):
    lo = j * (rows - span) // 16 + 17               # 16 distinct windows, none aligned to a work item
    return (lo, lo + span)


CASES = {
    "i_one_window": ([window(3)] * nq, [0] * nq),
    "ii_16_windows": ([window(q // max(1, nq // 16) % 16) for q in range(nq)], [0] * nq),
    "iii_default_filter": ([None] * nq, [0b111] * nq),
}


def form_a(ranges, denies):
    return [eng.searchFiltered(queries[q], k, timeRange=ranges[q], denyFlags=denies[q]) for q in range(nq)]


def form_b(ranges, denies):
    # the host's own filter: one pass over its columns per DISTINCT predicate, the list object shared by the queries that share it
    made = {}
    lists = []
    for q in range(nq):
        key = (ranges[q], denies[q])
        if key not in made:
            m = (flags & np.uint32(denies[q])) == 0
            if ranges[q] is not None:
                m &= (ts >= ranges[q][0]) & (ts < ranges[q][1])
            made[key] = ids[m]
        lists.append(made[key])
    return eng.searchBatchFiltered(queries, k, frameIds=lists)


def form_c(ranges, denies):
    return eng.searchBatchFiltered(queries, k, timeRange=ranges, denyFlags=denies)


def timed(fn, *a):
    t0 = time.perf_counter()
    fn(*a)
    return (time.perf_counter() - t0) * 1e3


out = {"rows": rows, "dims": dims, "topk": k, "queries": nq, "reps": args.reps, "cases": {}}
for name, (ranges, denies) in CASES.items():
    ref = form_a(ranges, denies)
    before = {key: eng.getTuning(key) for key in ("predicate_batch_queries", "predicate_batch_classes", "filter_batch_fallbacks")}
    st0 = eng.stats()
    got = form_c(ranges, denies)
    st1 = eng.stats()
    for q in range(nq):
        c = int(got[2][q])
        assert c == len(ref[q][0]) and np.array_equal(got[0][q, :c], ref[q][0]) and np.array_equal(got[1][q, :c], ref[q][1]), (name, q)
    b = form_b(ranges, denies)
    assert np.array_equal(b[0], got[0]) and np.array_equal(b[2], got[2]), name
    row = {key: eng.getTuning(key) - v for key, v in before.items()}
    assert row["predicate_batch_queries"] == nq and row["filter_batch_fallbacks"] == 0, row
    row["rows_read_by_the_gather"] = int(st1.rows_scanned - st0.rows_scanned)
    forms = {"a_loop_ms": form_a, "b_host_lists_ms": form_b, "c_batch_predicate_ms": form_c}
    t = {f: [] for f in forms}
    for _ in range(args.reps):
        for f, fn in forms.items():
            t[f].append(timed(fn, ranges, denies))
    row.update({f: round(statistics.median(v), 4) for f, v in t.items()})
    best = min(row["a_loop_ms"], row["b_host_lists_ms"])
    row["baseline"] = "a" if best == row["a_loop_ms"] else "b"
    row["c_speedup_over_baseline"] = round(best / row["c_batch_predicate_ms"], 3)
    out["cases"][name] = row
    print(json.dumps({name: row}), file=sys.stderr, flush=True)
print(json.dumps(out))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
eng.close()
