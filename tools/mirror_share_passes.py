#!/usr/bin/env python3
"""Time of ONE pass over the bf16 mirror and over the 8-bit code mirror by the number of queries it carries ("mirror_share" 2,
blocking collects), the two mirrors alternated ("mirror_bits" 16 / 8) in one process.

    python tools/mirror_share_passes.py [--rows 10000000] [--dims 384] [--reps 30] [--bits 16,8] [--out FILE]

A group of n = 1 .. 4 queries is submitted (parked), then collected: the first collect launches the one pass that answers all of
them, so wall time per group = upload + scan + finish + the host's wake-up, nothing overlapped. If the pass is still bound by HBM
the time per group stays where n = 1 has it; the line also gives the mirror bytes over that time (8 bits: rows x (dims + 8)). One
JSON line per (bits, n), and first one line with the wall time of the query that built the code mirror."""
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dims", type=int, default=384)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--bits", default="16,8", help="mirrors to time, alternated per n (a library without \"mirror_bits\": 16)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    eng = wax.HIPVectorEngine(dimensions=args.dims)
    eng.reserve(args.rows)
    for r0, x in bench.device_rows(torch, 0, args.rows, args.dims, dev):
        eng.addBatchDevice(np.arange(r0, r0 + x.shape[0], dtype=np.uint64), x)
    q = bench.unit_queries(64, args.dims)
    eng.setTuning("scan_mirror", 2)
    eng.setTuning("mirror_share", 2)
    eng.setTuning("slots", 4)
    lines = []
    bits_list = [int(b) for b in args.bits.split(",")]
    if 8 in bits_list:
        # the code mirror is built by the third eligible query in a row: its wall time against the next one's is the conversion
        eng.setTuning("mirror_bits", 8)
        walls = []
        for i in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.collect(eng.submit(q[i], args.k), args.k)
            walls.append(round((time.perf_counter() - t0) * 1e3, 3))
        line = {"rows": args.rows, "dims": args.dims, "first_five_queries_wall_ms": walls, "mirror8_conversions": eng.getTuning("mirror8_conversions"),
                "mirror8_rows_converted": eng.getTuning("mirror8_rows_converted"), "conversion_ms_about": round(walls[2] - walls[3], 3)}
        print(json.dumps(line), flush=True)
        lines.append(line)
    for n, bits in [(n, b) for n in (1, 2, 3, 4, 1) for b in bits_list]:
        if bits_list != [16]:
            eng.setTuning("mirror_bits", bits)
        def group(i):
            tickets = [eng.submit(q[(i * 4 + j) % 64], args.k) for j in range(n)]
            for t in tickets:
                eng.collect(t, args.k)
        for i in range(5):
            group(i)
        torch.cuda.synchronize()
        p0, f0 = eng.getTuning("mirror_passes"), eng.getTuning("mirror_scan_fallbacks")
        p8 = eng.getTuning("mirror8_passes") if bits == 8 else 0
        times = []
        for i in range(args.reps):
            t0 = time.perf_counter()
            group(i)
            times.append(time.perf_counter() - t0)
        passes = eng.getTuning("mirror_passes") - p0
        med = float(np.median(times))
        row_bytes = args.dims + 8 if bits == 8 else args.dims * 2
        line = {"rows": args.rows, "dims": args.dims, "mirror_bits": bits, "queries_per_pass": n,
                "passes_on_8_bits": eng.getTuning("mirror8_passes") - p8 if bits == 8 else 0, "groups": args.reps, "passes": passes,
                "fallbacks": eng.getTuning("mirror_scan_fallbacks") - f0,
                "ms_per_group_median": round(med * 1e3, 4), "ms_per_group_min": round(min(times) * 1e3, 4),
                "ms_per_group_iqr": round(float(np.subtract(*np.percentile(times, [75, 25]))) * 1e3, 4),
                "ms_per_query": round(med * 1e3 / n, 4), "mirror_TBps": round(args.rows * row_bytes / med / 1e12, 3)}
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
