#!/usr/bin/env python3
"""searchBatchResident against searchBatch on small stores, one blocking call at a time.

Legs: searchBatchResident, searchBatch — alternated call by call in one process on one engine, blocking wall time per call (every call
ends in a device synchronise), median and interquartile range of --reps per leg; np.array_equal of the two answers is asserted before
any timing. searchBatch is the baseline: this tool's subject does not change it. One JSON record.

    python tools/batch_resident_bench.py --out profiles/r36/batch_resident.json
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
    ap.add_argument("--rows", type=int, nargs="+", default=[1000, 3000, 8192, 16384, 32768, 65536])
    ap.add_argument("--dims", type=int, nargs="+", default=[384, 768])
    ap.add_argument("--nq", type=int, nargs="+", default=[32, 256, 1024])
    ap.add_argument("--topk", type=int, nargs="+", default=[10, 100])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import wax_amd
    torch.cuda.set_device(0)
    record = {"reps": args.reps, "cases": []}
    for dims in args.dims:
        queries = bench.unit_queries(max(args.nq), dims)
        for rows in args.rows:
            corpus = np.random.default_rng(rows + dims).standard_normal((rows, dims), dtype=np.float32)
            corpus /= np.linalg.norm(corpus, axis=1, keepdims=True)
            eng = wax_amd.HIPVectorEngine(metric=wax_amd.VectorMetric(0), dimensions=dims)
            eng.addBatch(np.arange(rows, dtype=np.uint64), corpus)
            for nq in args.nq:
                for k in args.topk:
                    q = np.ascontiguousarray(queries[:nq])
                    legs = {"resident": lambda: eng.searchBatchResident(q, k), "batch": lambda: eng.searchBatch(q, k)}
                    for _ in range(3):                                   # both legs warm: buffers allocated, mirrors built
                        got, want = legs["resident"](), legs["batch"]()
                    assert all(np.array_equal(a, b) for a, b in zip(got, want)), (rows, dims, nq, k)
                    times = {name: [] for name in legs}
                    for _ in range(args.reps):
                        for name, leg in legs.items():
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            leg()
                            times[name].append((time.perf_counter() - t0) * 1e6)
                    case = {"rows": rows, "dims": dims, "nq": nq, "top_k": k, "stats": eng.searchBatchResident(q, k, stats=True)[3],
                            **{name: quartiles(ts) for name, ts in times.items()}}
                    record["cases"].append(case)
                    print(json.dumps(case), flush=True)
            eng.close()
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
