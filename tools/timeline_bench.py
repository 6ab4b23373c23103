#!/usr/bin/env python3
"""The timeline lane (wax_hip_timeline) at --rows rows (default 10M, 64-d: the dimension is irrelevant to the lane).

For each timestamp column — ascending with row, descending with row, random, all equal — each limit of 30 / 300 / 1 000 and both
orders, medians of --reps:
  blocking_ms   one wax_hip_timeline call, wall clock (column check, two launches, one download, one synchronisation)
  device_ms     one wax_hip_timeline_device call between two events on its stream (both kernels and the markers around them)
  floor_ms      the bytes the scan must read over the stream-read rate wax_hip_time_stream_read gives on the same box in the same run:
                12 B per row (timestamp + flags) plus 8 B per row whose frame id must be loaded — the passing rows whose timestamp
                is not beyond the answer's last one (all of them when every timestamp is equal)
One JSON line per measurement; --out writes the whole record.

Kernel time comes from a kernel trace, in a run of its own: under
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/timeline_bench.py --device-only --plan-out PLAN
the tool issues exactly --reps device-form calls per configuration, in the order PLAN records, and
    python tools/timeline_bench.py --fold-trace DIR --plan PLAN --into RECORD
puts the median duration of timeline_select_kernel and timeline_merge_kernel per configuration into the record (select_us, merge_us).
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=10_000_000)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--out", default=None)
ap.add_argument("--device-only", action="store_true")
ap.add_argument("--plan-out", default=None)
ap.add_argument("--fold-trace", default=None)
ap.add_argument("--plan", default=None)
ap.add_argument("--into", default=None)
args = ap.parse_args()

LIMITS = (30, 300, 1000)
COLUMNS = ("ascending", "descending", "random", "equal")


def fold_trace():
    plan = json.load(open(args.plan))
    files = sorted(glob.glob(os.path.join(args.fold_trace, "**", "*kernel_trace.csv"), recursive=True))
    assert files, f"no kernel trace under {args.fold_trace}"
    rows = [r for f in files for r in csv.DictReader(open(f))]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    dur = {name: [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if name in r["Kernel_Name"]]
           for name in ("timeline_select_kernel", "timeline_merge_kernel")}
    reps, n_cfg = plan["reps"], len(plan["configs"])
    skip = plan["warmup_calls"]
    for name, d in dur.items():
        assert len(d) == skip + reps * n_cfg, (name, len(d), skip, reps, n_cfg)
    record = json.load(open(args.into))
    by_key = {(m["column"], m["limit"], m["newest_first"]): m for m in record["measurements"]}
    for i, cfg in enumerate(plan["configs"]):
        m = by_key[(cfg["column"], cfg["limit"], cfg["newest_first"])]
        for name, key in (("timeline_select_kernel", "select_us"), ("timeline_merge_kernel", "merge_us")):
            m[key] = round(statistics.median(dur[name][skip + i * reps: skip + (i + 1) * reps]), 2)
        print(json.dumps(m))
    record["kernel_trace"] = "rocprofv3 --kernel-trace: median dispatch duration per configuration"
    json.dump(record, open(args.into, "w"), indent=1)


if args.fold_trace:
    fold_trace()
    sys.exit(0)

import torch  # noqa: E402
import wax_amd as wax  # noqa: E402

torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
n, dims = args.rows, 64
rng = np.random.default_rng(1)
ids = np.arange(n, dtype=np.uint64) + 1
eng = wax.HIPVectorEngine(dimensions=dims)
eng.reserve(n)
chunk = 1 << 20
for r0 in range(0, n, chunk):                                   # rows made on the device: only their number matters here
    m = min(chunk, n - r0)
    eng.addBatchDevice(ids[r0:r0 + m], torch.randn((m, dims), dtype=torch.float32, device=dev))
torch.cuda.synchronize()

stream_ms = eng.timeStreamRead(10)
rate = n * dims * 4 / (stream_ms * 1e-3)                         # bytes per second
stream = torch.cuda.current_stream(dev).cuda_stream
record = {"rows": n, "dims": dims, "reps": args.reps, "stream_read_ms": stream_ms, "stream_read_gbps": rate / 1e9, "measurements": []}
plan = {"reps": args.reps, "warmup_calls": 0, "configs": []}


def column(kind):
    if kind == "ascending":
        return np.arange(n, dtype=np.int64) + 1_700_000_000_000
    if kind == "descending":
        return 1_700_000_000_000 + n - np.arange(n, dtype=np.int64)
    if kind == "random":
        return rng.integers(0, 1 << 40, size=n).astype(np.int64)
    return np.zeros(n, dtype=np.int64)


def ids_that_must_load(ts, limit, newest):
    """Passing rows (all pass here) whose timestamp is not beyond the answer's last one."""
    if limit >= n:
        return n
    if newest:
        kth = np.partition(ts, n - limit)[n - limit]
        return int(np.count_nonzero(ts >= kth))
    kth = np.partition(ts, limit - 1)[limit - 1]
    return int(np.count_nonzero(ts <= kth))


for kind in COLUMNS:
    ts = column(kind)
    eng.setAttributes(ids, ts, None)
    for limit in LIMITS:
        d_ids = torch.zeros(limit, dtype=torch.int64, device=dev)
        d_cnt = torch.zeros(1, dtype=torch.int32, device=dev)
        for newest in (True, False):
            cfg = {"column": kind, "limit": limit, "newest_first": newest}
            plan["configs"].append(cfg)
            if args.device_only:
                for _ in range(args.reps):
                    eng.timelineDevice(limit, d_ids, d_cnt, newest, stream=stream)
                torch.cuda.synchronize()
                continue
            got = eng.timeline(limit, newest)                    # warm: the columns are uploaded by the first call
            eng.timelineDevice(limit, d_ids, d_cnt, newest, stream=stream)
            torch.cuda.synchronize()
            assert np.array_equal(d_ids.cpu().numpy().view(np.uint64), got[0]) and len(got[0]) == limit
            wall, on_device = [], []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                eng.timeline(limit, newest)
                wall.append((time.perf_counter() - t0) * 1e3)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                eng.timelineDevice(limit, d_ids, d_cnt, newest, stream=stream)
                e1.record()
                e1.synchronize()
                on_device.append(e0.elapsed_time(e1))
            must = ids_that_must_load(ts, limit, newest)
            floor_ms = (12 * n + 8 * must) / rate * 1e3
            m = dict(cfg, blocking_ms=round(statistics.median(wall), 4), device_ms=round(statistics.median(on_device), 4),
                     floor_ms=round(floor_ms, 4), ids_that_must_load=must)
            m["blocking_over_floor"] = round(m["blocking_ms"] / floor_ms, 2)
            m["device_over_floor"] = round(m["device_ms"] / floor_ms, 2)
            record["measurements"].append(m)
            print(json.dumps(m), flush=True)
eng.close()
if args.plan_out:
    json.dump(plan, open(args.plan_out, "w"), indent=1)
if args.out and not args.device_only:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(record, open(args.out, "w"), indent=1)
