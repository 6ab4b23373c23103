#!/usr/bin/env python3
"""The routes of wax_hip_search_predicate against each other and against the unfiltered scans.

Store: --rows x 384 (default 1M), top-10, blocking calls, alternated runs, medians. For each pass fraction (1/64, 1/8, 1/2, 15/16)
and each mask shape (a random deny bit, one contiguous time range) it times the gather route ("predicate_route" 1), the masked
f32 scan (2 with "predicate_mirror" 0), the masked scan's mirror form (2 with "predicate_mirror" 2), today's alternative —
searchFiltered with the allow-list of the passing ids — and, in the same alternation, the unfiltered f32 scan ("scan_mirror" 0) and
the unfiltered lone bf16 mirror pass ("scan_mirror" 2, "mirror_bits" 16); "mirror_share" is 0 throughout. It prints one JSON line
and, with --out, writes the same object to a file: the route table with each form's run-to-run spread (the interquartile range of
its alternated times), the crossover of the random mask (the smallest measured fraction from which the masked f32 scan is faster than
the gather), the same for the mirror form, masked / unfiltered and mirror / masked at 15/16, and the bytes both scans read.

--pipelined N (default 4; 0 skips it) adds the pipelined legs under the product's own settings ("scan_mirror" 1, "mirror_share" 1,
"mirror_bits" 0, "predicate_route" 0, "predicate_mirror" 1): for a random mask passing 15/16, one passing 1/2 and a contiguous range
of 1/16 of the rows, the blocking predicate query (median of --reps calls) beside submitFiltered tickets with N in flight (time per
query over --pipelined-queries queries, and what predicateTicketStats() says became of them), and the unfiltered submit / collect
pair with N in flight. --skip-routes leaves the route table out (the pipelined legs alone, for alternated A/B runs at 10M rows). A
library without the ticket entry point reports null for the pipelined predicate legs."""
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
import torch  # noqa: E402
import wax_amd as wax  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--out", default=None)
ap.add_argument("--pipelined", type=int, default=4, help="queries in flight of the pipelined legs (0: no such legs)")
ap.add_argument("--pipelined-queries", type=int, default=400)
ap.add_argument("--skip-routes", action="store_true", help="leave the route table out")
args = ap.parse_args()

torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
rows, dims, k = args.rows, 384, 10
eng = wax.HIPVectorEngine(dimensions=dims)
eng.reserve(rows)
for r0, x in bench.device_rows(torch, 0, rows, dims, dev):
    eng.addBatchDevice(np.arange(r0, r0 + x.shape[0], dtype=np.uint64), x)
eng.setTuning("scan_mirror", 0)
eng.setTuning("mirror_share", 0)
eng.setTuning("mirror_bits", 16)
ids = np.arange(rows, dtype=np.uint64)
rng = np.random.default_rng(0)
# bit 8 + j: a random mask that PASSES fraction FRACS[j] (the bit is set on the rows that fail); timestamps ascend with the row
FRACS = [(1, 64), (1, 8), (1, 2), (15, 16)]
flags = np.zeros(rows, dtype=np.uint32)
u = rng.random(rows)
for j, (a, b) in enumerate(FRACS):
    flags[u >= a / b] |= np.uint32(1 << (8 + j))
eng.setAttributes(ids, ids.astype(np.int64), flags)
q = bench.unit_queries(4, dims)


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def alternated(fns, reps):
    """Every function once per round, in turn, `reps` rounds after one warm-up round: medians in ms, and under name + "_iqr" the
    interquartile range of the same times (the run-to-run spread a difference of medians has to exceed)."""
    for f in fns.values():
        f(0)
    t = {name: [] for name in fns}
    for i in range(reps):
        for name, f in fns.items():
            t[name].append(timed(lambda: f(i)))
    res = {name: round(statistics.median(v), 4) for name, v in t.items()}
    for name, v in t.items():
        qs = statistics.quantiles(v, n=4) if len(v) >= 2 else [v[0], v[0], v[0]]
        res[name.replace("_ms", "") + "_iqr_ms"] = round(qs[2] - qs[0], 4)
    return res


def routed(route, mirror=0, **kw):
    def f(i):
        eng.setTuning("predicate_route", route)
        eng.setTuning("predicate_mirror", mirror)
        got = eng.searchFiltered(q[i % 4], k, **kw)
        assert len(got[0]) == k
    return f


def unfiltered(scan_mirror):
    def f(i):
        eng.setTuning("scan_mirror", scan_mirror)
        got = eng.searchArrays(q[i % 4], k)
        assert len(got[0]) == k
    return f


def pipelined_legs(depth, n):
    """The blocking predicate query, predicate tickets with `depth` in flight and unfiltered tickets with `depth` in flight."""
    from collections import deque
    for key, value in (("scan_mirror", 1), ("mirror_share", 1), ("mirror_bits", 0), ("predicate_route", 0), ("predicate_mirror", 1)):
        eng.setTuning(key, value)
    qs = bench.unit_queries(64, dims)

    def pipeline(submit):
        """ms per query of n queries with `depth` in flight, after a warm-up of 8 * depth"""
        inflight = deque()
        t0 = 0.0
        for i in range(-8 * depth, n):
            if i == 0:
                while inflight:
                    eng.collect(inflight.popleft(), k)
                t0 = time.perf_counter()
            if len(inflight) == depth:
                got = eng.collect(inflight.popleft(), k)
                assert len(got[0]) == k
            inflight.append(submit(qs[i % 64]))
        while inflight:
            eng.collect(inflight.popleft(), k)
        return (time.perf_counter() - t0) * 1e3 / n

    legs = {"in_flight": depth, "queries": n, "masks": []}
    span = rows // 16
    lo = min(rows // 7, rows - span)
    for name, kw in (("random 15/16", {"denyFlags": 1 << (8 + FRACS.index((15, 16)))}), ("random 1/2", {"denyFlags": 1 << (8 + FRACS.index((1, 2)))}),
                     ("contiguous 1/16", {"timeRange": (lo, lo + span)})):
        eng.searchFiltered(qs[0], k, **kw)
        times = [timed(lambda i=i: eng.searchFiltered(qs[i % 64], k, **kw)) for i in range(max(args.reps, 5))]
        quart = statistics.quantiles(times, n=4)
        leg = {"mask": name, "blocking_ms": round(statistics.median(times), 4), "blocking_iqr_ms": round(quart[2] - quart[0], 4)}
        try:
            before = eng.predicateTicketStats()
            ms = pipeline(lambda v: eng.submitFiltered(v, k, **kw))
            after = eng.predicateTicketStats()
            leg.update({"pipelined_ms_per_query": round(ms, 4), "pipelined_over_blocking_rate": round(leg["blocking_ms"] / ms, 3),
                        "tickets": {key: after[key] - before[key] for key in after}})
        except wax.WaxError:
            leg.update({"pipelined_ms_per_query": None, "pipelined_over_blocking_rate": None, "tickets": None})
        legs["masks"].append(leg)
        print(json.dumps(leg), file=sys.stderr, flush=True)
    ms = pipeline(lambda v: eng.submit(v, k))
    legs["unfiltered_pipelined_ms_per_query"] = round(ms, 4)
    legs["unfiltered_pipelined_qps"] = round(1e3 / ms, 1)
    return legs


MIRROR_COUNTERS = ("predicate_mirror_scans", "predicate_mirror_fallbacks", "predicate_mirror_unavailable")
out = {"rows": rows, "dims": dims, "topk": k, "reps": args.reps, "table": []}


def emit(doc):
    print(json.dumps(doc))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    eng.close()


if args.skip_routes:
    out["pipelined"] = pipelined_legs(args.pipelined, args.pipelined_queries) if args.pipelined > 0 else None
    emit(out)
    sys.exit(0)
for a, b in [(1, 64), (1, 16), (1, 8), (1, 2), (15, 16)]:     # 1/16: the contiguous range only (what the chunk skip is for)
    span = rows * a // b
    lo = min(rows // 7, rows - span)
    shapes = [("contiguous", {"timeRange": (lo, lo + span)}, ids[lo:lo + span])]
    if (a, b) in FRACS:
        deny = 1 << (8 + FRACS.index((a, b)))
        shapes.insert(0, ("random", {"denyFlags": deny}, ids[(flags & np.uint32(deny)) == 0]))
    for shape, kw, passing in shapes:
        m0, s0 = eng.getTuning("predicate_masked_scans"), eng.getTuning("predicate_chunks_skipped")
        b0 = eng.stats().bytes_scanned
        routed(2, **kw)(0)
        scans = eng.getTuning("predicate_masked_scans") - m0
        row = {"pass": f"{a}/{b}", "mask": shape, "passing_rows": int(len(passing)),
               "masked_bytes_read": int(eng.stats().bytes_scanned - b0), "chunks_skipped": eng.getTuning("predicate_chunks_skipped") - s0}
        assert scans == 1
        c0 = [eng.getTuning(c) for c in MIRROR_COUNTERS]
        b0, s0 = eng.stats().bytes_scanned, eng.getTuning("predicate_chunks_skipped")
        routed(2, 2, **kw)(0)
        row["mirror_bytes_read"] = int(eng.stats().bytes_scanned - b0)        # (a fallback adds the f32 scan's bytes)
        row["mirror_chunks_skipped"] = eng.getTuning("predicate_chunks_skipped") - s0
        row.update(alternated({
            "gather_ms": routed(1, **kw),
            "masked_ms": routed(2, 0, **kw),
            "masked_mirror_ms": routed(2, 2, **kw),
            "allow_list_ms": lambda i, p=passing: eng.searchFiltered(q[i % 4], k, frameIds=p),
            "unfiltered_ms": unfiltered(0),
            "unfiltered_bf16_ms": unfiltered(2),
        }, args.reps))
        for c, v0 in zip(MIRROR_COUNTERS, c0):                                # over the probe, the warm-up and the timed rounds
            row[c] = eng.getTuning(c) - v0
        row["masked_over_unfiltered"] = round(row["masked_ms"] / row["unfiltered_ms"], 4)
        row["mirror_over_masked"] = round(row["masked_mirror_ms"] / row["masked_ms"], 4)
        row["mirror_over_unfiltered_bf16"] = round(row["masked_mirror_ms"] / row["unfiltered_bf16_ms"], 4)
        out["table"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
eng.setTuning("predicate_route", 0)
eng.setTuning("predicate_mirror", 1)
eng.setTuning("scan_mirror", 0)
rand = [r for r in out["table"] if r["mask"] == "random"]
# the crossover: the smallest measured fraction from which on the masked scan wins at every larger one too
cross = None
for r in rand:
    if all(x["masked_ms"] <= x["gather_ms"] for x in rand[rand.index(r):]):
        cross = r["pass"]
        break
out["random_mask_crossover_pass"] = cross
out["random_mask_crossover_permille"] = None if cross is None else int(round(1000 * int(cross.split("/")[0]) / int(cross.split("/")[1])))
out["masked_over_unfiltered_at_15_16"] = [r["masked_over_unfiltered"] for r in rand if r["pass"] == "15/16"][0]
# the same for the mirror form against the gather, and the decision figure: mirror / masked f32 at 15/16 beside both spreads
cross = None
for r in rand:
    if all(x["masked_mirror_ms"] <= x["gather_ms"] for x in rand[rand.index(r):]):
        cross = r["pass"]
        break
out["random_mask_mirror_crossover_pass"] = cross
at = [r for r in rand if r["pass"] == "15/16"][0]
out["mirror_over_masked_at_15_16"] = at["mirror_over_masked"]
out["mirror_faster_at_15_16_beyond_spread"] = bool(at["masked_ms"] - at["masked_mirror_ms"] > max(at["masked_iqr_ms"], at["masked_mirror_iqr_ms"]))
if args.pipelined > 0:
    out["pipelined"] = pipelined_legs(args.pipelined, args.pipelined_queries)
emit(out)
