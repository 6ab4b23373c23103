#!/usr/bin/env python3
"""searchMirrorL2 against the loop of search calls it replaces (searchArrays; searchFiltered under a mask) on an L2 store, with the
cosine engine's lone and four-query bf16 mirror passes over the same rows beside them as the floor.

Legs: loop, mirror_l2 — alternated call by call in one process on one engine, blocking wall time per call (every call ends in a device
synchronise), median and interquartile range of --reps per leg; np.array_equal of the two answers is asserted before any timing.
Masks: none, a random 15/16 and a random 1/2 of the rows, a contiguous 1/16 (flag bits). The floor: searchArrays on a cosine engine
with "scan_mirror" 2 and "mirror_bits" 16 (one bf16 pass per query), and four tickets submitted under "mirror_share" 2 and collected
(one shared pass). The loops and the cosine passes are baselines: this tool's subject does not change them. One JSON record.

    python tools/mirror_l2_bench.py --out profiles/r38/mirror_l2.json
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

MASKS = {"none": 0, "random 15/16": 1, "random 1/2": 2, "contiguous 1/16": 4}   # denyFlags


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
    ap.add_argument("--rows", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--dims", type=int, default=384)
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 4, 64])
    ap.add_argument("--topk", type=int, default=10)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import wax_amd
    torch.cuda.set_device(0)
    sync = torch.cuda.synchronize
    record = {"reps": args.reps, "cases": []}
    for rows in args.rows:
        rng = np.random.default_rng(rows + args.dims)
        l2 = wax_amd.HIPVectorEngine(metric=wax_amd.VectorMetric.l2, dimensions=args.dims)
        cos = wax_amd.HIPVectorEngine(metric=wax_amd.VectorMetric.cosine, dimensions=args.dims)
        for lo in range(0, rows, 1 << 20):                         # a slab at a time: the host never holds the whole corpus
            part = rng.standard_normal((min(1 << 20, rows - lo), args.dims), dtype=np.float32)
            part *= (rng.uniform(0.5, 1.0, (len(part), 1)) / np.linalg.norm(part, axis=1, keepdims=True)).astype(np.float32)
            for eng in (l2, cos):
                eng.addBatch(np.arange(lo, lo + len(part), dtype=np.uint64), part)
        draw = rng.integers(0, 16, rows)
        flags = (draw == 0).astype(np.uint32) | ((draw < 8).astype(np.uint32) << 1) | 4   # bit 0 on 1/16 of the rows, bit 1 on 1/2, bit 2 outside the window
        flags[rows // 2:rows // 2 + rows // 16] &= ~np.uint32(4)
        l2.setAttributes(np.arange(rows, dtype=np.uint64), np.arange(rows, dtype=np.int64), flags)
        queries = rng.standard_normal((max(args.nq), args.dims), dtype=np.float32)
        queries *= (rng.uniform(0.5, 1.0, (len(queries), 1)) / np.linalg.norm(queries, axis=1, keepdims=True)).astype(np.float32)
        for nq in args.nq:
            q = np.ascontiguousarray(queries[:nq])
            for name, deny in MASKS.items():
                one = (lambda v: l2.searchFiltered(v, args.topk, denyFlags=deny)) if deny else (lambda v: l2.searchArrays(v, args.topk))
                legs = {"loop": lambda: [one(v) for v in q], "mirror_l2": lambda: l2.searchMirrorL2(q, args.topk, denyFlags=deny)}
                for _ in range(3):                                   # every leg warm: buffers allocated, mirror and bitmap built
                    want, got = legs["loop"](), legs["mirror_l2"]()
                assert all(np.array_equal(got[0][i, :got[2][i]], w[0]) and np.array_equal(got[1][i, :got[2][i]], w[1]) for i, w in enumerate(want)), (rows, nq, name)
                case = {"rows": rows, "dims": args.dims, "nq": nq, "top_k": args.topk, "mask": name,
                        "stats": l2.searchMirrorL2(q, args.topk, denyFlags=deny, stats=True)[3], **timed(legs, args.reps, sync)}
                record["cases"].append(case)
                print(json.dumps(case), flush=True)
        # the floor: the cosine engine's bf16 passes over the same rows
        cos.setTuning("scan_mirror", 2)
        cos.setTuning("mirror_bits", 16)

        def four():
            cos.setTuning("mirror_share", 2)
            tickets = [cos.submit(v, args.topk) for v in queries[:4]]
            out = [cos.collect(t, args.topk) for t in tickets]
            cos.setTuning("mirror_share", 0)
            return out
        cos.setTuning("mirror_share", 0)
        legs = {"cosine_lone": lambda: cos.searchArrays(queries[0], args.topk), "cosine_four": four}
        for _ in range(3):
            legs["cosine_lone"](), legs["cosine_four"]()
        passes0, scans0 = cos.getTuning("mirror_passes"), cos.getTuning("mirror_scans")
        floor = timed(legs, args.reps, sync)
        case = {"rows": rows, "dims": args.dims, "top_k": args.topk, "floor": True, **floor,
                "mirror_passes": cos.getTuning("mirror_passes") - passes0, "mirror_scans": cos.getTuning("mirror_scans") - scans0}
        record["cases"].append(case)
        print(json.dumps(case), flush=True)
        l2.close()
        cos.close()
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
