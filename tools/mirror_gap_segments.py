#!/usr/bin/env python3
"""Where the time between two shared mirror passes goes, from one rocprofv3 trace with kernels and HIP calls.

    rocprofv3 --kernel-trace --hip-trace --output-format csv -d DIR -o t -- python bench.py --gpus 1 --steps 50 --warmup 10
    python tools/mirror_gap_segments.py DIR/.../t_kernel_trace.csv DIR/.../t_hip_api_trace.csv [--last 50] [--out FILE]

For every pair of consecutive passes (scan kernels as tools/mirror_pass_gaps.py finds them) the gap from the end of one scan to the
start of the next is cut at
    the start and the end of the finish kernel behind the first scan,
    the host's wake-up: the return of the first hipEventSynchronize that ends after the finish kernel (a build whose collect polls a
        word makes no such call: the start of the host's first HIP call after the finish kernel stands in for it),
    the start of the first call of the launch sequence of the next pass (the run of hipMemcpyAsync / hipEventRecord /
        hipLaunchKernel calls that ends with the launch of the next scan, query uploads included).
Medians over the pairs, microseconds. HIP calls cost more under the tracer than without it: the host legs are upper bounds, the
kernel legs are not affected. One JSON object."""
import argparse
import csv
import json
import re

import numpy as np

LAUNCH_CALLS = ("hipMemcpyAsync", "hipEventRecord", "hipLaunchKernel", "hipModuleLaunchKernel", "hipExtLaunchKernel", "hipExtModuleLaunchKernel",
                "hipGetLastError", "__hipPushCallConfiguration", "__hipPopCallConfiguration", "hipEventQuery", "hipStreamQuery")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("kernel_trace")
    ap.add_argument("hip_trace")
    ap.add_argument("--last", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    scans, finishes = [], []
    with open(args.kernel_trace, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"]
            rec = (int(row["Start_Timestamp"]), int(row["End_Timestamp"]), int(row["Correlation_Id"]))
            if re.search(r"mirror8?_scan_(group_)?kernel", name):
                scans.append(rec)
            elif re.search(r"mirror8?_finish_(group_)?kernel", name):
                finishes.append(rec)
    scans.sort()
    finishes.sort()
    calls = []
    with open(args.hip_trace, newline="") as f:
        for row in csv.DictReader(f):
            calls.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]), row["Function"], int(row["Correlation_Id"])))
    calls.sort()
    starts = np.array([c[0] for c in calls])
    by_corr = {c[3]: i for i, c in enumerate(calls)}
    if args.last > 0:
        scans = scans[-args.last:]
    seg = {k: [] for k in ("scan_end_to_finish_start", "finish_kernel", "finish_end_to_wake", "wake_to_launch_sequence", "launch_sequence_to_scan_start", "gap")}
    calls_in_launch = {}
    for a, b in zip(scans[:-1], scans[1:]):
        fin = next((f_ for f_ in finishes if a[0] <= f_[0] <= b[0]), None)
        li = by_corr.get(b[2])
        if fin is None or li is None:
            continue
        # the launch sequence: walk back from the launch of the next scan over launch-type calls that start after the finish began
        j = li
        while j > 0 and calls[j - 1][2] in LAUNCH_CALLS and calls[j - 1][0] >= fin[0]:
            j -= 1
        t_seq = calls[j][0]
        for c in calls[j:li + 1]:
            calls_in_launch[c[2]] = calls_in_launch.get(c[2], 0) + 1
        waits = [c for c in calls[int(np.searchsorted(starts, a[0])):li] if c[2] == "hipEventSynchronize" and c[1] >= fin[1]]
        if waits:
            t_wake = waits[0][1]
        else:
            k = int(np.searchsorted(starts, fin[1]))
            t_wake = calls[k][0] if k < len(calls) else fin[1]
        t_wake = min(t_wake, t_seq)
        seg["scan_end_to_finish_start"].append(fin[0] - a[1])
        seg["finish_kernel"].append(fin[1] - fin[0])
        seg["finish_end_to_wake"].append(t_wake - fin[1])
        seg["wake_to_launch_sequence"].append(t_seq - t_wake)
        seg["launch_sequence_to_scan_start"].append(b[0] - t_seq)
        seg["gap"].append(b[0] - a[1])
    n = len(seg["gap"])
    out = {"kernel_trace": args.kernel_trace, "pairs": n,
           "median_us": {k: round(float(np.median(v)) / 1e3, 2) for k, v in seg.items() if v},
           "p10_us": {k: round(float(np.percentile(v, 10)) / 1e3, 2) for k, v in seg.items() if v},
           "calls_per_launch_sequence": {k: round(v / max(n, 1), 2) for k, v in sorted(calls_in_launch.items())}}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
