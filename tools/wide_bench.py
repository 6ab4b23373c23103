#!/usr/bin/env python3
"""searchWide against search(topK=k) for the k UnifiedSearch sends (candidateLimit: 72, 300, 1 000), one blocking query at a time.

Legs: searchWide(bits=8), searchWide(bits=16), search(topK=k) — alternated query by query in one process, blocking wall time per
call (every call ends in a device synchronise), median of --reps per leg; the certified share over --queries queries; the floor of
each mirror leg = the pass's bytes over the stream-read rate this run measures (wax_hip_time_stream_read). One JSON record.

    python tools/wide_bench.py --rows 10000000 --dims 384 --out profiles/r35/wide.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dims", type=int, default=384)
    ap.add_argument("--topk", type=int, nargs="+", default=[72, 300, 1000])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    eng = bench._load_engine(torch, dev, args.rows, args.dims)
    qs = bench.unit_queries(max(args.queries, args.reps) + 4, args.dims)
    legs = {"wide8": lambda q, k: eng.searchWide(q, k, bits=8), "wide16": lambda q, k: eng.searchWide(q, k, bits=16),
            "search": lambda q, k: eng.searchArrays(q, k)}
    gbps = args.rows * args.dims * 4 / (eng.timeStreamRead(10) * 1e-3) / 1e9      # the f32 store over its read-only pass
    record = {"rows": args.rows, "dims": args.dims, "reps": args.reps, "stream_read_gbps": gbps, "by_k": {}}
    for k in args.topk:
        for q in qs[:4]:                                   # every leg warm at this k (mirrors built, buffers allocated)
            for leg in legs.values():
                leg(q, k)
        times = {name: [] for name in legs}
        for q in qs[4:4 + args.reps]:
            for name, leg in legs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                leg(q, k)
                times[name].append((time.perf_counter() - t0) * 1e3)
        row = {"ms_median": {n: statistics.median(t) for n, t in times.items()}, "ms_min": {n: min(t) for n, t in times.items()}}
        for bits in (8, 16):
            stats = [eng.searchWide(q, k, bits=bits, stats=True)[2] for q in qs[:args.queries]]
            row[f"certified_share_{bits}"] = sum(s["certified"] for s in stats) / len(stats)
            row[f"candidates_median_{bits}"] = statistics.median(s["candidates"] for s in stats)
            row[f"bound_sources_{bits}"] = [sum(s["bound_source"] == i for s in stats) for i in range(3)]
            pass_bytes = args.rows * (args.dims + 8 if bits == 8 else args.dims * 2)
            row[f"floor_ms_{bits}"] = pass_bytes / (gbps * 1e9) * 1e3
        same = all((a == b).all() for q in qs[:8] for a, b in zip(eng.searchWide(q, k, bits=8), eng.searchArrays(q, k)))
        row["equal_to_search"] = bool(same)
        record["by_k"][str(k)] = row
        print(json.dumps({"top_k": k, **row}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
