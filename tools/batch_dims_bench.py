#!/usr/bin/env python3
"""searchBatchDims (the K-split register-resident filtering GEMM) against searchBatch (the LDS-tiled one) at 1 024 and 1 536 dimensions.

Legs: dims, batch — alternated call by call in one process on one engine, blocking wall time per call, median and interquartile range
of --reps per leg; np.array_equal of the two answers is asserted before any timing. The filtering GEMM's own time comes from the
"time_kernels" statistics, each leg in a run of --reps calls of its own behind the wall-time legs. Floor per case:
max(2 Q N D / 2.5 PFLOP/s, N D 2 B / the stream-read rate wax_hip_time_stream_read gives in the same run). One JSON record.

    python tools/batch_dims_bench.py --out profiles/r40/batch_dims.json
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

SHAPES = ((1_000_000, 1024), (650_000, 1536))


def quartiles(ts):
    q = statistics.quantiles(ts, n=4)
    return {"median_us": statistics.median(ts), "iqr_us": q[2] - q[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--topk", type=int, default=10)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import wax_amd
    torch.cuda.set_device(0)
    record = {"reps": args.reps, "cases": []}
    for rows, dims in SHAPES:
        rng = np.random.default_rng(rows + dims)
        eng = wax_amd.HIPVectorEngine(metric=wax_amd.VectorMetric(0), dimensions=dims)
        for lo in range(0, rows, 1 << 18):                         # a slab at a time: the host never holds the whole corpus
            part = rng.standard_normal((min(1 << 18, rows - lo), dims), dtype=np.float32)
            part /= np.linalg.norm(part, axis=1, keepdims=True)
            eng.addBatch(np.arange(lo, lo + len(part), dtype=np.uint64), part)
        gbps = rows * dims * 4 / (eng.timeStreamRead(10) * 1e-3) / 1e9      # the f32 store over its read-only pass
        for nq in args.nq:
            q = np.ascontiguousarray(bench.unit_queries(nq, dims))
            legs = {"dims": lambda: eng.searchBatchDims(q, args.topk), "batch": lambda: eng.searchBatch(q, args.topk)}
            for _ in range(3):                                       # both legs warm: buffers allocated, mirror built
                got, want = legs["dims"](), legs["batch"]()
            assert all(np.array_equal(a, b) for a, b in zip(got, want)), (rows, dims, nq)
            times = {leg: [] for leg in legs}
            for _ in range(args.reps):
                for leg, call in legs.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    call()
                    times[leg].append((time.perf_counter() - t0) * 1e6)
            gemm = {}
            eng.setTuning("time_kernels", 1)
            for leg, call in legs.items():
                eng.setTuning("reset_stats", 1)
                for _ in range(args.reps):
                    call()
                st = eng.stats()
                gemm[leg] = st.batch_gemm_ms_total / st.batch_gemms_timed * 1e3 if st.batch_gemms_timed else float("nan")
            eng.setTuning("time_kernels", 0)
            floor_us = max(2.0 * nq * rows * dims / 2.5e15, rows * dims * 2 / (gbps * 1e9)) * 1e6
            case = {"rows": rows, "dims": dims, "nq": nq, "top_k": args.topk, "stream_read_gbps": gbps, "floor_us": floor_us,
                    "stats": eng.searchBatchDims(q, args.topk, stats=True)[3],
                    **{leg: dict(quartiles(ts), gemm_us=gemm[leg]) for leg, ts in times.items()}}
            case["gemm_ratio_dims_over_batch"] = gemm["dims"] / gemm["batch"]
            case["wall_ratio_dims_over_batch"] = case["dims"]["median_us"] / case["batch"]["median_us"]
            record["cases"].append(case)
            print(json.dumps(case), flush=True)
        eng.close()
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
