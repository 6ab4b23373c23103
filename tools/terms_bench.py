#!/usr/bin/env python3
"""The required-term search against what a caller of the parent commit does.

Store: --rows x 384 (default 10M), cosine, top-10, blocking calls, the two legs alternated in one process, medians of --reps (15).
Every row holds six terms: ONE session id and five terms of its own. The sessions are assigned at random: session 0 owns 1/2 of the
rows, session 1 owns 1/16, session 2 owns 1/1 000, the rest is spread over a thousand small sessions — so one column serves the three
session sizes.
  leg (a)  today's alternative: a numpy filter of the HOST session column gives the passing ids, searchFiltered(frameIds=...)
           follows; the host time is part of the leg.
  leg (b)  searchFiltered(requiredTerms=[the session's term]).
Both legs must return the same arrays (asserted once per size). It prints one JSON line and, with --out, writes the same object:
per size the medians, the interquartile ranges, (a) / (b), and what termStats() and the route counters say (b) did; the store's
stream-read rate from wax_hip_time_stream_read in the same run and term_mask_kernel's byte floor 4 (rows + 1) + 4 total_terms.

--trace-leg SIZE runs only leg (b) of that size --reps times and then the stream read, and writes rows, floor and stream rate to
--out (for `rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/terms_bench.py --trace-leg 1000 --out T.json`);
`--trace-csv DIR/.../kernel_trace.csv --out T.json` (no GPU) then adds term_mask_kernel's median duration from that trace and the
rate at which it read its floor, beside the stream rate of the same run."""
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
ap.add_argument("--trace-leg", type=int, default=0, help="1000, 16 or 2: only leg (b) of that session size")
ap.add_argument("--trace-csv", default=None, help="a rocprofv3 kernel_trace.csv of a --trace-leg run")
args = ap.parse_args()



def iqr(xs):
    qs = statistics.quantiles(xs, n=4)
    return qs[2] - qs[0]


if args.trace_csv:
    with open(args.out) as f:
        doc = json.load(f)
    with open(args.trace_csv) as f:
        durs = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in csv.DictReader(f) if "term_mask_" in r["Kernel_Name"]]
    durs = durs[3:] if len(durs) > 3 else durs                  # the first calls upload the column and warm the caches
    med = statistics.median(durs)
    doc["term_mask_kernel_us"] = {"n": len(durs), "median": med, "min": min(durs), "max": max(durs), "iqr": iqr(durs) if len(durs) > 3 else None}
    doc["term_mask_kernel_gbps_of_floor"] = doc["term_mask_floor_bytes"] / med / 1e3
    doc["term_mask_kernel_over_floor_at_stream_rate"] = med / doc["term_mask_floor_us_at_stream_rate"]
    print(json.dumps(doc))
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    sys.exit(0)

import bench  # noqa: E402
import torch  # noqa: E402
import wax_amd as wax  # noqa: E402

torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
rows, dims, k = args.rows, 384, 10
SIZES = (1000, 16, 2)
WHICH = {2: 0, 16: 1, 1000: 2}                                    # the session that owns 1 / size of the rows
SESSION_BASE = 10_000
eng = wax.HIPVectorEngine(dimensions=dims)
eng.reserve(rows)
for r0, x in bench.device_rows(torch, 0, rows, dims, dev):
    eng.addBatchDevice(np.arange(r0, r0 + x.shape[0], dtype=np.uint64), x)
ids = np.arange(rows, dtype=np.uint64)
rng = np.random.default_rng(0)
u = rng.random(rows)
session = np.where(u < 0.5, 0, np.where(u < 0.5 + 1 / 16, 1, np.where(u < 0.5 + 1 / 16 + 1 / 1000, 2, 3 + rng.integers(0, 1000, size=rows)))).astype(np.uint32)   # the host column leg (a) filters
terms = np.empty((rows, 6), dtype=np.uint32)
terms[:, 0] = SESSION_BASE + session
terms[:, 1:] = 1_000_000 + 5 * np.arange(rows, dtype=np.uint32)[:, None] + np.arange(5, dtype=np.uint32)[None, :]
t0 = time.perf_counter()
for r0 in range(0, rows, 1_000_000):
    eng.setTerms(ids[r0:r0 + 1_000_000], terms[r0:r0 + 1_000_000])
set_s = time.perf_counter() - t0
q = np.random.default_rng(1).standard_normal(dims).astype(np.float32)


def leg_a(s, which):
    allow = ids[session == which]
    return eng.searchFiltered(q, k, frameIds=allow)


def leg_b(s, which):
    return eng.searchFiltered(q, k, requiredTerms=[SESSION_BASE + which])


def stream_fields(doc):
    stream_ms = eng.timeStreamRead(20)
    store_bytes = rows * dims * 4
    floor_bytes = 4 * (rows + 1) + 4 * int(terms.size)
    doc["stream_read_ms"] = stream_ms
    doc["stream_read_gbps"] = store_bytes / stream_ms / 1e6
    doc["term_mask_floor_bytes"] = floor_bytes
    doc["term_mask_floor_us_at_stream_rate"] = floor_bytes / (store_bytes / stream_ms / 1e3)


def emit(doc):
    print(json.dumps(doc))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if args.trace_leg:
    for _ in range(args.reps + 3):
        leg_b(args.trace_leg, WHICH[args.trace_leg])
    doc = {"rows": rows, "dims": dims, "terms_per_row": 6, "trace_leg": f"1/{args.trace_leg}", "calls": args.reps + 3}
    stream_fields(doc)
    emit(doc)
    sys.exit(0)

COUNTERS = ("predicate_gather_searches", "predicate_masked_scans", "predicate_mirror_scans", "predicate_mirror_fallbacks")
out = {"rows": rows, "dims": dims, "k": k, "reps": args.reps, "terms_per_row": 6, "set_terms_seconds": set_s, "sizes": {}}
for s in SIZES:
    a, b = leg_a(s, WHICH[s]), leg_b(s, WHICH[s])                              # warm: the column's upload, the id table
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32)) and len(b[0]) == k
    c0 = {c: eng.getTuning(c) for c in COUNTERS}
    st0 = eng.termStats()
    ta, tb = [], []
    for _ in range(args.reps):
        t = time.perf_counter(); leg_a(s, WHICH[s]); ta.append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter(); leg_b(s, WHICH[s]); tb.append((time.perf_counter() - t) * 1e3)
    st1 = eng.termStats()
    out["sizes"][f"1/{s}"] = {
        "passing_rows": int((session == WHICH[s]).sum()),
        "a_host_filter_then_allow_list_ms": statistics.median(ta), "a_iqr_ms": iqr(ta),
        "b_required_terms_ms": statistics.median(tb), "b_iqr_ms": iqr(tb),
        "a_over_b": statistics.median(ta) / statistics.median(tb),
        "b_counters": {c: eng.getTuning(c) - c0[c] for c in COUNTERS},
        "b_term_stats": {key: st1[key] - st0[key] for key in st1},
    }
stream_fields(out)
emit(out)
