#!/usr/bin/env python3
"""The grouped search (wax_hip_search_grouped) at --rows x 384 cosine (default 10M), limit 12, blocking wall time, medians
of --reps, every leg alternated with the others in one process:

  singleton_p1 / _p3   the store before any parent is set: one group per row, every row an atomic on a slot of its own
  grouped_p1 / _p3     roots of ~10 rows (--layout contiguous: rows r // 10 share a root; scattered: a random assignment)
  search_top10         (a) the blocking f32 search, top-10, "scan_mirror" 0: the floor — the fused scan reads the same bytes plus 8-12 B a row
  overfetch_p1 / _p3   (b) what a caller does today: search(topK = max(400, 8 * limit * per_group)) and the collapse by root on the host

The first --crowd rows of the store are the query plus a little noise and share ONE root (the long video whose segments all resemble
the query): `overfetch_differs` counts the roots of leg (b) that are not the exact answer's, position by position.

One JSON line per leg; --out writes the record.

Kernel time comes from a kernel trace, one leg per run:
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/grouped_bench.py --trace-leg grouped_p3
issues 2 warm-up calls and --reps calls of that leg alone, and
    python tools/grouped_bench.py --fold-trace DIR --trace-leg grouped_p3 --into RECORD
adds, per kernel name, the microseconds per call (all launches of that kernel in a call summed; the warm-up calls left out).
"""
import argparse
import csv
import glob
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
ap.add_argument("--layout", default="contiguous", choices=("contiguous", "scattered"))
ap.add_argument("--crowd", type=int, default=600)
ap.add_argument("--out", default=None)
ap.add_argument("--trace-leg", default=None)
ap.add_argument("--fold-trace", default=None)
ap.add_argument("--into", default=None)
args = ap.parse_args()

LIMIT, WARM = 12, 2
KERNELS = ("group_fill_kernel", "group_scan_kernel", "group_offer_kernel", "group_split_kernel", "timeline_select_kernel",
           "timeline_merge_kernel", "group_mark_kernel", "group_round_kernel", "group_advance_kernel", "group_ids_kernel", "scan_kernel",
           "merge_keys_kernel", "attr_mask_kernel")


def fold_trace():
    files = sorted(glob.glob(os.path.join(args.fold_trace, "**", "*kernel_trace.csv"), recursive=True))
    assert files, f"no kernel trace under {args.fold_trace}"
    rows = [r for f in files for r in csv.DictReader(open(f))]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    calls = WARM + args.reps
    out = {}
    for name in KERNELS:
        d = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows
             if r["Kernel_Name"].split("(")[0].split("<")[0].split("::")[-1].strip() == name]
        if not d or len(d) % calls:
            continue                                             # (a kernel of the store's build, not of the leg)
        per = len(d) // calls
        out[name] = {"launches_per_call": per, "us_per_call": round(sum(d[WARM * per:]) / args.reps, 2)}
    record = json.load(open(args.into))
    record.setdefault("kernel_trace", {})[args.trace_leg] = out
    json.dump(record, open(args.into, "w"), indent=1)
    print(json.dumps({args.trace_leg: out}))


if args.fold_trace:
    fold_trace()
    sys.exit(0)

import torch  # noqa: E402
import wax_amd as wax  # noqa: E402

torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
n, dims = args.rows, 384
rng = np.random.default_rng(1)
ids = np.arange(n, dtype=np.uint64) + 1
q = rng.standard_normal(dims).astype(np.float32)
eng = wax.HIPVectorEngine(dimensions=dims)
eng.setTuning("scan_mirror", 0)
eng.reserve(n)
chunk = 1 << 20
torch.manual_seed(1)
for r0 in range(0, n, chunk):
    m = min(chunk, n - r0)
    rows = torch.randn((m, dims), dtype=torch.float32, device=dev)
    if r0 == 0:                                                  # the crowd: the query plus a little noise
        c = min(args.crowd, m)
        rows[:c] = torch.from_numpy(q).to(dev)[None, :] + 0.05 * torch.randn((c, dims), dtype=torch.float32, device=dev)
    eng.addBatchDevice(ids[r0:r0 + m], rows)
torch.cuda.synchronize()

per_root = 10
if args.layout == "contiguous":
    group = np.arange(n, dtype=np.uint64) // np.uint64(per_root)
else:
    group = rng.permutation(n).astype(np.uint64) // np.uint64(per_root)
parents = np.uint64(1 << 40) + group
parents[:args.crowd] = np.uint64(1 << 41)                        # one root owns the best rows


def over_fetch(per_group):
    top_k = max(400, 8 * LIMIT * per_group)
    got, scores = eng.searchArrays(q, top_k)
    roots = parents[(got - np.uint64(1)).astype(np.int64)]       # the caller's own metadata lookup
    best = {}
    for r, s in zip(roots.tolist(), scores.tolist()):
        if r not in best:
            best[r] = s                                          # best first: the first hit of a root is its score
    ranked = sorted(best.items(), key=lambda kv: (-kv[1], kv[0]))[:LIMIT]
    return np.array([r for r, _ in ranked], dtype=np.uint64)


LEGS = {
    "singleton_p1": lambda: eng.searchGrouped(q, LIMIT, 1),
    "singleton_p3": lambda: eng.searchGrouped(q, LIMIT, 3),
    "grouped_p1": lambda: eng.searchGrouped(q, LIMIT, 1),
    "grouped_p3": lambda: eng.searchGrouped(q, LIMIT, 3),
    "search_top10": lambda: eng.searchArrays(q, 10),
    "overfetch_p1": lambda: over_fetch(1),
    "overfetch_p3": lambda: over_fetch(3),
}


def run(names, record):
    wall = {k: [] for k in names}
    for k in names:
        for _ in range(WARM):
            LEGS[k]()
    for _ in range(args.reps):                                   # alternated: one call of every leg per round
        for k in names:
            t0 = time.perf_counter()
            LEGS[k]()
            wall[k].append((time.perf_counter() - t0) * 1e3)
    for k in names:
        m = {"leg": k, "blocking_ms": round(statistics.median(wall[k]), 4), "min_ms": round(min(wall[k]), 4), "max_ms": round(max(wall[k]), 4)}
        record["measurements"].append(m)
        print(json.dumps(m), flush=True)


record = {"rows": n, "dims": dims, "metric": "cosine", "limit": LIMIT, "reps": args.reps, "layout": args.layout, "crowd": args.crowd,
          "rows_per_root": per_root, "measurements": []}

if args.trace_leg:
    if not args.trace_leg.startswith(("singleton", "search")):
        eng.setParents(ids, parents)
    for _ in range(WARM + args.reps):
        LEGS[args.trace_leg]()
    eng.close()
    sys.exit(0)

run(("singleton_p1", "singleton_p3", "search_top10"), record)
t0 = time.perf_counter()
assert eng.setParents(ids, parents) == n
record["set_parents_s"] = round(time.perf_counter() - t0, 3)
t0 = time.perf_counter()
exact1 = eng.searchGrouped(q, LIMIT, 1)                          # the first grouped search numbers the roots and uploads the slot column
record["first_grouped_search_s"] = round(time.perf_counter() - t0, 3)
run(("grouped_p1", "grouped_p3", "search_top10", "overfetch_p1", "overfetch_p3"), record)
for per_group in (1, 3):
    exact = eng.searchGrouped(q, LIMIT, per_group)[0]
    today = over_fetch(per_group)
    differs = sum(1 for i in range(LIMIT) if i >= len(today) or today[i] != exact[i])
    m = {"leg": f"overfetch_p{per_group}", "top_k": max(400, 8 * LIMIT * per_group), "overfetch_roots": int(len(today)), "exact_roots": int(len(exact)),
         "overfetch_differs": differs}
    record["measurements"].append(m)
    print(json.dumps(m), flush=True)
record["group_stats"] = eng.groupStats()
eng.close()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(record, open(args.out, "w"), indent=1)
