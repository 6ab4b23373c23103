#!/usr/bin/env python3
"""searchMirror against the loop of search calls it replaces (searchArrays; searchFiltered under a mask) on cosine stores at 512, 1 024
and 1 536 dimensions whose f32 image is about 15 GB each, with the byte floor of the passes beside every figure.

Legs: loop, mirror, codes (searchMirror(bits=8): the 8-bit code mirror on the int8 matrix pipe) — alternated call by call in one process on one engine, blocking wall time per call (every call ends in a device
synchronise), median and interquartile range of --reps per leg; np.array_equal of the answers is asserted before any timing.
Masks: none, a random 15/16 of the rows, a contiguous 1/16 (flag bits). floor_us: the bf16 bytes the passes read (rows outside the
chunks the call reports as skipped, 2 B per element, once per pass) over the stream-read rate wax_hip_time_stream_read gives in the
same run on the same store; floor8_us: the same for the codes leg, D + 8 bytes per row of the 16-row tiles it reads. stats, stats8: the call's own words — how many queries certified, how many were re-run. One JSON record.

    python tools/mirror_dims_bench.py --out profiles/r42/mirror8_dims.json
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

MASKS = {"none": 0, "random 15/16": 1, "contiguous 1/16": 2}   # denyFlags
CHUNK_ROWS = {512: 8, 1024: 4, 1536: 4}                        # rows per wave iteration of the pass: the unit of the bitmap's skip
SLAB = 1 << 18


def quartiles(ts):
    q = statistics.quantiles(ts, n=4)
    return {"median_us": statistics.median(ts), "iqr_us": q[2] - q[0]}


def timed(legs, reps, sync):
    times = {leg: [] for leg in legs}
    for _ in range(reps):
        for leg, call in legs.items():
            sync()
            t0 = time.perf_counter()
            call()
            times[leg].append((time.perf_counter() - t0) * 1e6)
    return {leg: quartiles(ts) for leg, ts in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, nargs="+", default=[512, 1024, 1536])
    ap.add_argument("--bytes", type=float, default=15.36e9, help="f32 image of each store (rows = bytes / (4 dims))")
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 4, 64])
    ap.add_argument("--topk", type=int, default=10)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--masks", nargs="+", default=list(MASKS), choices=list(MASKS))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import wax_amd
    torch.cuda.set_device(0)
    sync = torch.cuda.synchronize
    record = {"reps": args.reps, "cases": []}
    for dims in args.dims:
        rows = int(args.bytes / (4 * dims))
        rng = np.random.default_rng(rows + dims)
        eng = wax_amd.HIPVectorEngine(metric=wax_amd.VectorMetric.cosine, dimensions=dims)
        # one slab of Gaussian directions; every further slab is the same rows under another random sign per element, which is as
        # far from the first (and from a query) as a fresh draw and spares the host 15 GB of normal deviates
        base = rng.standard_normal((min(SLAB, rows), dims), dtype=np.float32)
        base /= np.linalg.norm(base, axis=1, keepdims=True)
        for lo in range(0, rows, SLAB):
            signs = rng.choice(np.array([-1.0, 1.0], dtype=np.float32), dims)
            eng.addBatch(np.arange(lo, min(lo + SLAB, rows), dtype=np.uint64), base[:min(SLAB, rows - lo)] * signs)
        flags = (rng.integers(0, 16, rows) == 0).astype(np.uint32) | 2   # bit 0 on 1/16 of the rows, bit 1 outside the window
        flags[rows // 2:rows // 2 + rows // 16] &= ~np.uint32(2)
        eng.setAttributes(np.arange(rows, dtype=np.uint64), np.arange(rows, dtype=np.int64), flags)
        queries = rng.standard_normal((max(args.nq), dims), dtype=np.float32)
        gbps = rows * dims * 4 / (eng.timeStreamRead(10) * 1e-3) / 1e9      # the f32 store over its read-only pass
        for nq in args.nq:
            q = np.ascontiguousarray(queries[:nq])
            for name, deny in ((m, MASKS[m]) for m in args.masks):
                one = (lambda v: eng.searchFiltered(v, args.topk, denyFlags=deny)) if deny else (lambda v: eng.searchArrays(v, args.topk))
                legs = {"loop": lambda: [one(v) for v in q], "mirror": lambda: eng.searchMirror(q, args.topk, denyFlags=deny),
                        "codes": lambda: eng.searchMirror(q, args.topk, denyFlags=deny, bits=8)}
                for _ in range(2):                                   # every leg warm: buffers allocated, mirror and bitmap built
                    want, got, got8 = legs["loop"](), legs["mirror"](), legs["codes"]()
                for g in (got, got8):
                    assert all(np.array_equal(g[0][i, :g[2][i]], w[0]) and np.array_equal(g[1][i, :g[2][i]], w[1]) for i, w in enumerate(want)), (dims, nq, name)
                stats = eng.searchMirror(q, args.topk, denyFlags=deny, returnStats=True)[3]
                stats8 = eng.searchMirror(q, args.topk, denyFlags=deny, returnStats=True, bits=8)[3]
                read = stats["passes"] * rows - stats["chunks_skipped"] * CHUNK_ROWS[dims]
                read8 = stats8["passes"] * rows - stats8["tiles_skipped"] * 16
                case = {"rows": rows, "dims": dims, "nq": nq, "top_k": args.topk, "mask": name, "stats": stats, "stats8": stats8, "stream_read_gbps": gbps,
                        "floor_us": read * dims * 2 / (gbps * 1e9) * 1e6, "floor8_us": read8 * (dims + 8) / (gbps * 1e9) * 1e6,
                        **timed(legs, args.reps, sync)}
                record["cases"].append(case)
                print(json.dumps(case), flush=True)
        eng.close()
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
