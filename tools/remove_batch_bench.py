#!/usr/bin/env python3
"""removeBatch against the remove loop. Builds two identical seeded engines and times, alternating, three repeats:

  batch        removeBatch of `--ids` random frame ids (engine A)
  single       ONE remove of the lowest listed row (engine B): the yardstick — it moves the same tail through the same two copies
  loop         the remove loop over the same ids (engine B); only a `--loop-prefix` of it where the whole loop would run for
               minutes, and then the figure for all ids is an EXTRAPOLATION and reported as such

Host clock around the blocking calls (every one of them ends synchronised). After a repeat the removed rows are appended again to
both engines, so every repeat starts from the same row count (the rows' order differs between repeats: the timing does not depend
on it). Prints one JSON record; --out also writes it to a file.

  python tools/remove_batch_bench.py --rows 1000000 --dims 384 --ids 1000
  python tools/remove_batch_bench.py --rows 10000000 --dims 384 --ids 10000 --loop-prefix 100
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rows_chunk(seed, lo, hi, dims):
    rng = np.random.default_rng([seed, lo])
    x = rng.standard_normal((hi - lo, dims), dtype=np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dims", type=int, default=384)
    ap.add_argument("--ids", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--loop-prefix", type=int, default=0, help="time only this many ids of the loop and extrapolate (0 = the whole loop)")
    ap.add_argument("--no-mirror", action="store_true", help="do not build the bf16 mirror first")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import wax_amd
    chunk = 250_000
    engines = [wax_amd.HIPVectorEngine(metric=wax_amd.VectorMetric.cosine, dimensions=a.dims) for _ in range(2)]
    for e in engines:
        e.reserve(a.rows + a.ids)
    for lo in range(0, a.rows, chunk):
        hi = min(a.rows, lo + chunk)
        x = rows_chunk(a.seed, lo, hi, a.dims)
        for e in engines:
            e.addBatch(np.arange(lo, hi, dtype=np.uint64), x)
    queries = rows_chunk(a.seed + 1, 0, 64, a.dims)

    def warm(e):
        if not a.no_mirror:
            e.searchBatch(queries, 10)       # the mirror (and whatever appended rows it lacks) is in place before the clock starts
        e.searchArrays(queries[0], 10)

    rng = np.random.default_rng(a.seed + 2)
    A, B = engines
    next_id = a.rows
    present = np.arange(a.rows, dtype=np.uint64)
    rec = {"tool": "remove_batch_bench", "rows": a.rows, "dims": a.dims, "ids": a.ids, "mirror": not a.no_mirror,
           "loop_prefix": a.loop_prefix, "repeats": []}
    for rep in range(a.repeats):
        for e in engines:
            warm(e)
        lst = rng.choice(present, size=a.ids, replace=False)
        listed = np.isin(present, lst)                       # `present`: the engines' frame ids in row order
        lowest = int(present[int(np.argmax(listed))])        # the lowest listed row's id
        w0 = A.getTuning("remove_batch_bytes_written")
        t0 = time.perf_counter()
        removed = A.removeBatch(lst)
        t_batch = time.perf_counter() - t0
        assert removed == a.ids, (removed, a.ids)
        written = A.getTuning("remove_batch_bytes_written") - w0
        t0 = time.perf_counter()
        B.remove(lowest)
        t_single = time.perf_counter() - t0
        rest = [int(v) for v in lst if int(v) != lowest]
        m = len(rest) if a.loop_prefix <= 0 else min(a.loop_prefix, len(rest))
        t0 = time.perf_counter()
        for v in rest[:m]:
            B.remove(v)
        t_loop = time.perf_counter() - t0
        if m < len(rest):
            B.removeBatch(np.array(rest[m:], dtype=np.uint64))      # untimed: bring B to the same state
        assert A.count == B.count == a.rows - a.ids
        per_id = t_loop / max(m, 1)
        r = {"batch_ms": t_batch * 1e3, "single_remove_ms": t_single * 1e3, "batch_over_single": t_batch / t_single,
             "loop_ids_timed": m + 1, "loop_timed_ms": (t_loop + t_single) * 1e3,
             "loop_all_ids_ms": (t_single + per_id * len(rest)) * 1e3, "loop_all_ids_extrapolated": m < len(rest),
             "bytes_written": int(written)}
        r["loop_over_batch"] = r["loop_all_ids_ms"] / r["batch_ms"]
        rec["repeats"].append(r)
        # refill: the same number of new rows at the end of both engines
        x = rows_chunk(a.seed + 3 + rep, 0, a.ids, a.dims)
        new = np.arange(next_id, next_id + a.ids, dtype=np.uint64)
        next_id += a.ids
        for e in engines:
            e.addBatch(new, x)
        present = np.concatenate([present[~listed], new])
    for key in ("batch_ms", "single_remove_ms", "batch_over_single", "loop_all_ids_ms", "loop_over_batch"):
        rec["median_" + key] = float(np.median([r[key] for r in rec["repeats"]]))
    rec["loop_all_ids_extrapolated"] = any(r["loop_all_ids_extrapolated"] for r in rec["repeats"])
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    for e in engines:
        e.close()


if __name__ == "__main__":
    main()
