#!/usr/bin/env python3
"""Passes over the bf16 mirror or the 8-bit code mirror in a rocprofv3 kernel trace: how many queries each carried and how long the GPU had no pass running.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- python bench.py --gpus 1
    python tools/mirror_pass_gaps.py DIR/.../NAME_kernel_trace.csv [--last 50] [--out FILE]

A pass is one dispatch of mirror_scan_kernel / mirror8_scan_kernel (one query) or of mirror_scan_group_kernel /
mirror8_scan_group_kernel<DIMS, METRIC, NQ> (NQ queries); "passes_on_8_bits" counts the latter kind, "mirror8_kernel_ms" lists the
conversions of the code mirror with the index of the pass they precede (a conversion in the timed region would show up here). The gap
behind a pass is the time from its end to the start of the next pass (negative: the two overlapped on their streams). --last N
looks at the last N passes only (the timed region of a bench run sits at the end of the trace). One JSON object."""
import argparse
import csv
import json
import re

import numpy as np


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("trace")
    ap.add_argument("--last", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    passes = []     # (start ns, end ns, queries, bits)
    builds = []     # (start ns, ms) of mirror8_kernel
    with open(args.trace, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"]
            m = re.search(r"mirror(8?)_scan_(group_)?kernel", name)
            if m is None:
                if "mirror8_kernel" in name:
                    builds.append((int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e6))
                continue
            nq = int(re.findall(r"\d+", name[name.index("<") + 1:name.index(">")])[-1]) if m.group(2) else 1   # <DIMS, METRIC, NQ>
            passes.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]), nq, 8 if m.group(1) else 16))
    passes.sort()
    total = len(passes)
    build_info = [{"ms": round(ms, 3), "before_pass": sum(1 for p in passes if p[0] < t), "of_passes": total} for t, ms in sorted(builds)]
    if args.last > 0:
        passes = passes[-args.last:]
    by_nq = {}
    for _, _, nq, _ in passes:
        by_nq[nq] = by_nq.get(nq, 0) + 1
    dur = {nq: [(e - s) / 1e6 for s, e, n, _ in passes if n == nq] for nq in by_nq}
    gaps = np.array([(passes[i + 1][0] - passes[i][1]) / 1e6 for i in range(len(passes) - 1)]) if len(passes) > 1 else np.zeros(0)
    span = (passes[-1][1] - passes[0][0]) / 1e6 if passes else 0.0
    out = {"trace": args.trace, "passes": len(passes), "queries": sum(n for _, _, n, _ in passes),
           "passes_on_8_bits": sum(1 for p in passes if p[3] == 8), "mirror8_kernel_ms": build_info,
           "passes_by_queries": {str(k): v for k, v in sorted(by_nq.items())},
           "pass_ms_median_by_queries": {str(k): round(float(np.median(v)), 4) for k, v in sorted(dur.items())},
           "span_ms": round(span, 3), "queries_per_second_over_span": round(sum(n for _, _, n, _ in passes) / span * 1e3, 1) if span else None,
           "sequence_tail": [n for _, _, n, _ in passes[-24:]]}
    if len(gaps):
        out["gap_ms"] = {k: round(float(v), 4) for k, v in (("min", gaps.min()), ("p10", np.percentile(gaps, 10)), ("median", np.median(gaps)),
                                                           ("p90", np.percentile(gaps, 90)), ("max", gaps.max()), ("mean", gaps.mean()))}
        out["gaps_negative"] = int((gaps < 0).sum())
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
