#!/usr/bin/env python3
"""searchBatchL2 (the register-resident L2 filtering GEMM) against searchBatch (the LDS-tiled one) on L2 stores at 384 and 768 dimensions.

Legs: l2, batch — alternated call by call in one process on one engine, blocking wall time per call, median and interquartile range
of --reps per leg; np.array_equal of the two answers is asserted before any timing. The filtering GEMM's own time comes from the
"time_kernels" statistics, each leg in a run of --reps calls of its own behind the wall-time legs. Beside them `cosine`: searchBatch of
a cosine store of the same rows — batch_gemm_rq_kernel, the register-resident kernel without the norm term, the figure the new launch
should approach. Rows are Gaussian directions with norms spread over [0.5, 1.0]. One JSON record.

    python tools/batch_l2_bench.py --out profiles/r41/batch_l2.json
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

SHAPES = ((1_000_000, 384, (256, 1024)), (1_250_000, 768, (1024,)))
COS, L2 = 0, 2


def quartiles(ts):
    q = statistics.quantiles(ts, n=4)
    return {"median_us": statistics.median(ts), "iqr_us": q[2] - q[0]}


def shell_rows(rng, n, dims):
    v = rng.standard_normal((n, dims), dtype=np.float32)
    return v * (rng.uniform(0.5, 1.0, (n, 1)).astype(np.float32) / np.linalg.norm(v, axis=1, keepdims=True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--topk", type=int, default=10)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import wax_amd
    torch.cuda.set_device(0)
    record = {"reps": args.reps, "cases": []}
    for rows, dims, batches in SHAPES:
        engs = {m: wax_amd.HIPVectorEngine(metric=wax_amd.VectorMetric(m), dimensions=dims) for m in (L2, COS)}
        rng = np.random.default_rng(rows + dims)
        for lo in range(0, rows, 1 << 18):                         # a slab at a time: the host never holds the whole corpus
            part = shell_rows(rng, min(1 << 18, rows - lo), dims)
            for eng in engs.values():
                eng.addBatch(np.arange(lo, lo + len(part), dtype=np.uint64), part)
        for nq in batches:
            q = np.ascontiguousarray(shell_rows(np.random.default_rng(nq), nq, dims))
            legs = {"l2": lambda: engs[L2].searchBatchL2(q, args.topk), "batch": lambda: engs[L2].searchBatch(q, args.topk),
                    "cosine": lambda: engs[COS].searchBatch(q, args.topk)}
            for _ in range(3):                                       # every leg warm: buffers allocated, mirrors built
                got, want, _cos = legs["l2"](), legs["batch"](), legs["cosine"]()
            assert all(np.array_equal(a, b) for a, b in zip(got, want)), (rows, dims, nq)
            times = {leg: [] for leg in legs}
            for _ in range(args.reps):
                for leg, call in legs.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    call()
                    times[leg].append((time.perf_counter() - t0) * 1e6)
            gemm = {}
            for leg, call in legs.items():                           # the filtering launch on its own
                eng = engs[COS if leg == "cosine" else L2]
                eng.setTuning("time_kernels", 1)
                eng.setTuning("reset_stats", 1)
                for _ in range(args.reps):
                    call()
                st = eng.stats()
                gemm[leg] = st.batch_gemm_ms_total / st.batch_gemms_timed * 1e3 if st.batch_gemms_timed else float("nan")
                eng.setTuning("time_kernels", 0)
            case = {"rows": rows, "dims": dims, "nq": nq, "top_k": args.topk, "stats": engs[L2].searchBatchL2(q, args.topk, stats=True)[3],
                    **{leg: dict(quartiles(ts), gemm_us=gemm[leg]) for leg, ts in times.items()}}
            case["gemm_ratio_l2_over_batch"] = gemm["l2"] / gemm["batch"]
            case["gemm_ratio_l2_over_cosine"] = gemm["l2"] / gemm["cosine"]
            case["wall_ratio_l2_over_batch"] = case["l2"]["median_us"] / case["batch"]["median_us"]
            record["cases"].append(case)
            print(json.dumps(case), flush=True)
        for eng in engs.values():
            eng.close()
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
