#!/usr/bin/env python3
"""The batched required-term search against the loop a caller of the parent commit writes.

Store: --rows x 384 (default 10M), cosine, top-10, blocking calls, the two legs alternated in one process, medians of --reps (15) with
interquartile ranges. Every row holds six terms: one of 1 000 SMALL sessions (1/1 000 of the rows each), one of 16 sessions of family A
and one of 16 of family B (1/16 of the rows each: 32 large sessions), and three terms of its own. A point is 256 queries drawn
round-robin from 8 or 32 sessions of one size.
  leg (a)  what the parent commit offers: the loop of searchFiltered(requiredTerms=[the query's session]).
  leg (b)  searchBatchTerms(queries, k, [...]): one call.
Both legs must return the same arrays (asserted once per point). It prints one JSON line and, with --out, writes the same object: per
point the medians, the interquartile ranges, (a) / (b), what termBatchStats() says (b) did, and the stream-read rate of the same run.

--trace-leg runs, for S = 1, 4 and 32 small sessions, --reps batched calls of S queries (one term_mask_multi_kernel launch each) and
then --reps single calls (term_mask_kernel), and then the stream read; under
`rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/batch_terms_bench.py --trace-leg --out T.json` the trace holds
their durations in that order. `--trace-csv DIR/.../kernel_trace.csv --out T.json` (no GPU) adds, per S, term_mask_multi_kernel's
median, S times term_mask_kernel's median, and the multi kernel's byte floor (the column and S bitmaps) at the stream rate."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=10_000_000)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--out", default=None)
ap.add_argument("--trace-leg", action="store_true", help="only the kernels' legs at S = 1, 4, 32, for a kernel trace")
ap.add_argument("--trace-csv", default=None, help="a rocprofv3 kernel_trace.csv of a --trace-leg run")
args = ap.parse_args()
TRACE_S = (1, 4, 32)
WARM = 2


def iqr(xs):
    qs = statistics.quantiles(xs, n=4)
    return qs[2] - qs[0]


def emit(doc):
    print(json.dumps(doc))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if args.trace_csv:
    with open(args.out) as f:
        doc = json.load(f)
    multi, single = [], []
    with open(args.trace_csv) as f:
        for r in sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"])):
            d = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
            if "term_mask_multi_kernel" in r["Kernel_Name"]:
                multi.append(d)
            elif "term_mask_kernel" in r["Kernel_Name"]:
                single.append(d)
    per = doc["calls_per_s"]
    assert len(multi) == per * len(TRACE_S), (len(multi), per)
    one = statistics.median(single)
    doc["term_mask_kernel_us"] = {"n": len(single), "median": one, "iqr": iqr(single)}
    doc["multi"] = {}
    for i, s in enumerate(TRACE_S):
        durs = multi[i * per + WARM:(i + 1) * per]
        med = statistics.median(durs)
        floor_us = (doc["column_bytes"] + s * doc["bitmap_bytes"]) / (doc["stream_read_gbps"] * 1e3)
        doc["multi"][str(s)] = {"n": len(durs), "median_us": med, "iqr_us": iqr(durs), "s_single_launches_us": s * one,
                                "single_over_multi": s * one / med, "floor_us_at_stream_rate": floor_us, "over_floor": med / floor_us}
    emit(doc)
    sys.exit(0)

import bench  # noqa: E402
import torch  # noqa: E402
import wax_amd as wax  # noqa: E402

torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
rows, dims, k, nq = args.rows, 384, 10, 256
SMALL0, A0, B0 = 10_000, 20_000, 30_000
eng = wax.HIPVectorEngine(dimensions=dims)
eng.reserve(rows)
for r0, x in bench.device_rows(torch, 0, rows, dims, dev):
    eng.addBatchDevice(np.arange(r0, r0 + x.shape[0], dtype=np.uint64), x)
ids = np.arange(rows, dtype=np.uint64)
rng = np.random.default_rng(0)
terms = np.empty((rows, 6), dtype=np.uint32)
terms[:, 0] = SMALL0 + rng.integers(0, 1000, size=rows)
terms[:, 1] = A0 + rng.integers(0, 16, size=rows)
terms[:, 2] = B0 + rng.integers(0, 16, size=rows)
terms[:, 3:] = 1_000_000 + 3 * np.arange(rows, dtype=np.uint32)[:, None] + np.arange(3, dtype=np.uint32)[None, :]
t0 = time.perf_counter()
for r0 in range(0, rows, 1_000_000):
    eng.setTerms(ids[r0:r0 + 1_000_000], terms[r0:r0 + 1_000_000])
set_s = time.perf_counter() - t0
queries = np.random.default_rng(1).standard_normal((nq, dims)).astype(np.float32)
SESSIONS = {"1/1000": [SMALL0 + i for i in range(32)], "1/16": [A0 + i for i in range(16)] + [B0 + i for i in range(16)]}


def stream_fields(doc):
    stream_ms = eng.timeStreamRead(20)
    doc["stream_read_ms"] = stream_ms
    doc["stream_read_gbps"] = rows * dims * 4 / stream_ms / 1e6
    doc["column_bytes"] = 4 * (rows + 1) + 4 * int(terms.size)
    doc["bitmap_bytes"] = 4 * ((rows + 31) // 32)


def leg_a(qs, req):
    return [eng.searchFiltered(qs[i], k, requiredTerms=req[i]) for i in range(len(qs))]


def leg_b(qs, req):
    return eng.searchBatchTerms(qs, k, req)


if args.trace_leg:
    per = args.reps + WARM
    for s in TRACE_S:
        req = [[SMALL0 + i] for i in range(s)]
        for _ in range(per):
            leg_b(queries[:s], req)
    for _ in range(per):
        leg_a(queries[:1], [[SMALL0]])
    doc = {"rows": rows, "dims": dims, "terms_per_row": 6, "calls_per_s": per, "trace_s": list(TRACE_S)}
    stream_fields(doc)
    emit(doc)
    sys.exit(0)

out = {"rows": rows, "dims": dims, "k": k, "queries": nq, "reps": args.reps, "terms_per_row": 6, "set_terms_seconds": set_s, "points": {}}
for size, pool in SESSIONS.items():
    for n_ses in (8, 32):
        req = [[pool[i % n_ses]] for i in range(nq)]
        a, b = leg_a(queries, req), leg_b(queries, req)                        # warm: the column's upload, the workspaces
        for i in range(nq):
            c = int(b[2][i])
            assert c == k and np.array_equal(a[i][0], b[0][i, :c]) and np.array_equal(a[i][1].view(np.int32), b[1][i, :c].view(np.int32)), (size, n_ses, i)
        st0 = eng.termBatchStats()
        ta, tb = [], []
        for _ in range(args.reps):
            t = time.perf_counter(); leg_a(queries, req); ta.append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter(); leg_b(queries, req); tb.append((time.perf_counter() - t) * 1e3)
        st1 = eng.termBatchStats()
        out["points"][f"{size} x {n_ses} sessions"] = {
            "a_loop_ms": statistics.median(ta), "a_iqr_ms": iqr(ta), "b_batched_ms": statistics.median(tb), "b_iqr_ms": iqr(tb),
            "a_over_b": statistics.median(ta) / statistics.median(tb),
            "b_term_batch_stats": {key: st1[key] - st0[key] for key in st1},
        }
stream_fields(out)
emit(out)
