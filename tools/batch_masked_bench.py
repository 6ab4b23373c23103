#!/usr/bin/env python3
"""searchBatchMasked against searchBatchFiltered with the same predicate, and against the unfiltered searchBatch as the floor.

Legs: masked, filtered, batch — alternated call by call in one process on one engine, blocking wall time per call (every call ends in
a device synchronise), median and interquartile range of --reps per leg; np.array_equal of the masked and the filtered answer is
asserted before any timing. Masks: a random 15/16 and a random 1/2 of the rows (flag bits), a contiguous 1/16 (a time range).
searchBatchFiltered and searchBatch are baselines: this tool's subject does not change them. One JSON record.

    python tools/batch_masked_bench.py --out profiles/r37/batch_masked.json
"""
from __future__ import annotations

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


def quartiles(ts):
    q = statistics.quantiles(ts, n=4)
    return {"median_us": statistics.median(ts), "iqr_us": q[2] - q[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--dims", type=int, default=384)
    ap.add_argument("--nq", type=int, default=256)
    ap.add_argument("--topk", type=int, default=10)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import wax_amd
    torch.cuda.set_device(0)
    record = {"reps": args.reps, "cases": []}
    q = np.ascontiguousarray(bench.unit_queries(args.nq, args.dims))
    for rows in args.rows:
        rng = np.random.default_rng(rows + args.dims)
        eng = wax_amd.HIPVectorEngine(metric=wax_amd.VectorMetric(0), dimensions=args.dims)
        for lo in range(0, rows, 1 << 20):                         # a slab at a time: the host never holds the whole corpus
            part = rng.standard_normal((min(1 << 20, rows - lo), args.dims), dtype=np.float32)
            part /= np.linalg.norm(part, axis=1, keepdims=True)
            eng.addBatch(np.arange(lo, lo + len(part), dtype=np.uint64), part)
        draw = rng.integers(0, 16, rows)
        flags = (draw == 0).astype(np.uint32) | ((draw < 8).astype(np.uint32) << 1)   # bit 0 on 1/16 of the rows, bit 1 on 1/2
        eng.setAttributes(np.arange(rows, dtype=np.uint64), np.arange(rows, dtype=np.int64), flags)
        masks = {"random 15/16": dict(denyFlags=1), "random 1/2": dict(denyFlags=2),
                 "contiguous 1/16": dict(timeRange=(rows // 2, rows // 2 + rows // 16))}
        for name, pred in masks.items():
            legs = {"masked": lambda: eng.searchBatchMasked(q, args.topk, **pred),
                    "filtered": lambda: eng.searchBatchFiltered(q, args.topk, **pred),
                    "batch": lambda: eng.searchBatch(q, args.topk)}
            for _ in range(3):                                       # every leg warm: buffers allocated, mirror and bitmap built
                got, want, _ = legs["masked"](), legs["filtered"](), legs["batch"]()
            assert all(np.array_equal(a, b) for a, b in zip(got, want)), (rows, name)
            times = {leg: [] for leg in legs}
            for _ in range(args.reps):
                for leg, call in legs.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    call()
                    times[leg].append((time.perf_counter() - t0) * 1e6)
            case = {"rows": rows, "dims": args.dims, "nq": args.nq, "top_k": args.topk, "mask": name,
                    "stats": eng.searchBatchMasked(q, args.topk, stats=True, **pred)[3], **{leg: quartiles(ts) for leg, ts in times.items()}}
            record["cases"].append(case)
            print(json.dumps(case), flush=True)
        eng.close()
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
