#!/usr/bin/env python3
"""Batched filtered search (wax_hip_search_batch_filtered) against the loop of searchFiltered calls it replaces.

Workloads (256 queries, cosine top-10): a = 1M x 384, per-query lists of 10 000 ids; b = 1M x 384, one shared list of 100 000;
c = 1M x 384, per-query lists of 100 ids; d = 10M x 384, per-query lists of 10 000 ids; x = 1M x 384, one shared list of the
given fraction of the store, against unfiltered searchBatch (the crossover). For each: ms per batch of the batched call
("filter_batch" 1), of the same call with "filter_batch" 0 (per-query path) and of the Python loop, with every answer asserted
equal, plus the rows the gather pass reads. Run under `rocprofv3 --kernel-trace --stats` (--only NAME, --reps N) for kernel
times; the gathered-bytes rate is rows x dims x 4 / the scan_multi_kernel time.

    python tools/filtered_batch_bench.py [--only a,b,c,d,x] [--reps 10] [--out FILE.json]
"""
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

NQ, K, DIMS = 256, 10, 384


def build_engine(rows):
    dev = torch.device("cuda", 0)
    eng = wax.HIPVectorEngine(dimensions=DIMS)
    eng.reserve(rows)
    for r0, x in bench.device_rows(torch, 0, rows, DIMS, dev):
        eng.addBatchDevice(np.arange(r0, r0 + x.shape[0], dtype=np.uint64), x)
    return eng


def timed(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    return out, (time.perf_counter() - t0) / reps * 1e3


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def run(eng, rows, lists, reps, loop_reps):
    q = bench.unit_queries(NQ, DIMS)
    res = {}
    eng.setTuning("filter_batch", 1)
    fused, res["batch_ms"] = timed(lambda: eng.searchBatchFiltered(q, K, frameIds=lists), reps)
    eng.setTuning("filter_batch", 0)
    per_query, res["batch_filter_batch_0_ms"] = timed(lambda: eng.searchBatchFiltered(q, K, frameIds=lists), loop_reps)
    eng.setTuning("filter_batch", 1)
    assert same(fused, per_query), "filter_batch 1 and 0 disagree"

    def loop():
        return [eng.searchFiltered(q[i], K, frameIds=lists[i]) for i in range(NQ)]
    ref, res["loop_ms"] = timed(loop, loop_reps)
    for i in range(NQ):
        c = int(fused[2][i])
        assert c == len(ref[i][0]) and np.array_equal(fused[0][i, :c], ref[i][0]) and np.array_equal(fused[1][i, :c], ref[i][1]), i
    distinct = {id(x): len(np.unique(x[x < rows])) for x in lists}
    per_pass = sum(distinct[id(x)] for x in {id(x): x for x in lists}.values())
    # queries of one list share a pass in groups of 16
    groups = {}
    for x in lists:
        groups[id(x)] = groups.get(id(x), 0) + 1
    gathered_rows = sum(distinct[k] * ((n + 15) // 16) for k, n in groups.items())
    res.update(distinct_lists=len(distinct), allowed_rows_distinct=per_pass, gathered_rows_per_batch=gathered_rows,
               gathered_bytes_per_batch=gathered_rows * DIMS * 4, speedup_vs_loop=round(res["loop_ms"] / res["batch_ms"], 2),
               answers_equal=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="a,b,c,d,x")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    only = set(args.only.split(","))
    torch.cuda.set_device(0)
    rng = np.random.default_rng(0)
    out = {"nq": NQ, "topk": K, "dims": DIMS, "metric": "cosine"}
    if only & {"a", "b", "c", "x"}:
        rows = 1_000_000
        eng = build_engine(rows)
        if "a" in only:
            lists = [rng.integers(0, rows, 10_000, dtype=np.uint64) for _ in range(NQ)]
            out["a_1m_per_query_10k"] = run(eng, rows, lists, args.reps, 2)
        if "b" in only:
            shared = rng.choice(rows, 100_000, replace=False).astype(np.uint64)
            out["b_1m_shared_100k"] = run(eng, rows, [shared] * NQ, args.reps, 2)
        if "c" in only:
            lists = [rng.integers(0, rows, 100, dtype=np.uint64) for _ in range(NQ)]
            out["c_1m_per_query_100"] = run(eng, rows, lists, args.reps, 2)
        if "x" in only:   # one shared list of a growing share of the store against unfiltered searchBatch
            q = bench.unit_queries(NQ, DIMS)
            _, unf = timed(lambda: eng.searchBatch(q, K), args.reps)
            cross = {"unfiltered_searchBatch_ms": round(unf, 4)}
            for frac in (1 / 64, 1 / 32, 1 / 16, 1 / 8, 1 / 4):
                shared = rng.choice(rows, int(rows * frac), replace=False).astype(np.uint64)
                _, ms = timed(lambda: eng.searchBatchFiltered(q, K, frameIds=[shared] * NQ), args.reps)
                cross[f"shared_{frac:.4f}_ms"] = round(ms, 4)
            out["x_crossover_1m_shared_list_256q"] = cross
        eng.close()
    if "d" in only:
        rows = 10_000_000
        eng = build_engine(rows)
        lists = [rng.integers(0, rows, 10_000, dtype=np.uint64) for _ in range(NQ)]
        out["d_10m_per_query_10k"] = run(eng, rows, lists, args.reps, 1)
        eng.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
