#!/usr/bin/env python3
"""The headline loop (bench.py's run_pipelined: collect the oldest ticket, submit one) with the mirror counters over its timed region.

    python tools/mirror_fill_counters.py [--label this] [--fill -1 0] [--reps 3] [--steps 200] [--warmup 20] [--depth 4] [--out FILE]
    WAX_HIP_LIB=<a build of another commit> python tools/mirror_fill_counters.py --label parent --fill -1

One store (10M x 384 by default, bench.py's rows and queries, two streams, `depth` slots), then per --fill value and repeat: warm-up,
a device barrier, `steps` timed steps, a barrier; the deltas of mirror_scans / mirror_passes / mirror_shared_passes /
mirror_shared_queries / mirror_scan_fallbacks / mirror_fill_holds are those of the timed steps alone. --fill -1 leaves "mirror_fill"
at the library's default (and is the only value a library without the key takes); a counter the library does not know reads 0.
One JSON line per run."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import torch  # noqa: E402
import wax_amd as wax  # noqa: E402

COUNTERS = ("mirror_scans", "mirror_passes", "mirror_shared_passes", "mirror_shared_queries", "mirror_scan_fallbacks", "mirror_fill_holds")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--label", default="this")
    ap.add_argument("--fill", type=int, nargs="+", default=[-1])
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dims", type=int, default=384)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    eng = wax.HIPVectorEngine(dimensions=args.dims)
    eng.reserve(args.rows)
    for r0, x in bench.device_rows(torch, 0, args.rows, args.dims, dev):
        eng.addBatchDevice(np.arange(r0, r0 + x.shape[0], dtype=np.uint64), x)
    torch.cuda.synchronize()
    q = bench.unit_queries(args.warmup + args.steps, args.dims)
    eng.setTuning("streams", 2)
    eng.setTuning("slots", max(args.depth, 2))

    def counter(name):
        try:
            return int(eng.getTuning(name))
        except Exception:
            return 0

    def submit(x):
        return eng.submit(x, args.k)

    def collect(t):
        return eng.collect(t, args.k)

    lines = []
    for fill in args.fill:
        if fill >= 0:
            eng.setTuning("mirror_fill", fill)
        for rep in range(args.reps):
            bench.run_pipelined(submit, collect, q[:args.warmup], args.depth)
            torch.cuda.synchronize()
            c0 = {c: counter(c) for c in COUNTERS}
            t0 = time.perf_counter()
            bench.run_pipelined(submit, collect, q[args.warmup:args.warmup + args.steps], args.depth)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            line = {"build": args.label, "mirror_fill": fill, "rep": rep, "steps": args.steps, "depth": args.depth,
                    "qps": round(args.steps / dt, 1), "ms_per_step": round(dt / args.steps * 1e3, 4)}
            line.update({c: counter(c) - c0[c] for c in COUNTERS})
            print(json.dumps(line), flush=True)
            lines.append(line)
    eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
