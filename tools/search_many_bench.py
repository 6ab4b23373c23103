#!/usr/bin/env python3
"""One query each against many small stores: wax_hip_search_many against the two ways of doing it per store.

--stores stores (default 256) of --rows rows x 384 on one device (defaults: 10 000, 50 000 and 174 762, the vec segment cap), one
query per store, cosine, top-30 (what Wax.search(topK: 10) asks the engine for). Three forms, alternated, medians of --reps:
  (a) loop_ms       one blocking wax_hip_search per store                                  — baseline
  (b) pipelined_ms  the same through wax_hip_search_submit / _collect, four in flight      — baseline
  (c) many_ms       one wax_hip_search_many                                                — the new call
It checks once that (c) returns what (a) returns, prints one JSON line per size and, with --out, writes the whole object to a file.

--predicate measures wax_hip_search_many_predicate instead: --stores stores of 10 000 rows (the first entry of --rows when given),
every pair with denyFlags = 0b111 (the default FrameFilter()), in two cases — 1/16 of the rows flagged at random, and the flagged rows
one contiguous quarter of the store, so whole chunks are clear. Three forms, alternated, medians of --reps:
  (a) filtered_loop_ms   one wax_hip_search_predicate per store (searchFiltered)   — the path before this call existed: the baseline
  (b) many_filtered_ms   one wax_hip_search_many_predicate (searchManyFiltered)
  (c) many_ms            one wax_hip_search_many on the same stores, unfiltered     — what the mask costs on top
It checks once that (b) returns what (a) returns and reports b/a and b/c per case."""
import argparse
import ctypes
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
ap.add_argument("--rows", default=None)
ap.add_argument("--predicate", action="store_true")
ap.add_argument("--stores", type=int, default=256)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--depth", type=int, default=4)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if args.rows is None:
    args.rows = "10000" if args.predicate else "10000,50000,174762"

torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
dims, k, n_stores = 384, 30, args.stores
queries = bench.unit_queries(n_stores, dims)


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def build_stores(rows):
    engines = []
    for j in range(n_stores):
        eng = wax.HIPVectorEngine(dimensions=dims)
        eng.reserve(rows)
        for r0, x in bench.device_rows(torch, j * rows, (j + 1) * rows, dims, dev):     # every store its own rows
            eng.addBatchDevice(np.arange(r0 - j * rows, r0 - j * rows + x.shape[0], dtype=np.uint64), x)
        engines.append(eng)
    return engines


def predicate_mode():
    from wax_amd import _abi
    rows, deny = int(args.rows.split(",")[0]), 0b111
    res = {"dims": dims, "topk": k, "stores": n_stores, "rows": rows, "reps": args.reps, "deny_flags": deny, "cases": []}
    engines = build_stores(rows)
    L = engines[0]._lib
    f32, u64 = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint64)
    a_ids, a_scores = np.zeros((n_stores, k), np.uint64), np.zeros((n_stores, k), np.float32)
    a_counts = np.zeros(n_stores, np.uint32)
    got = ctypes.c_uint32(0)
    hs = [e._h for e in engines]
    qp = [queries[j].ctypes.data_as(f32) for j in range(n_stores)]
    ip = [a_ids[j].ctypes.data_as(u64) for j in range(n_stores)]
    sp = [a_scores[j].ctypes.data_as(f32) for j in range(n_stores)]
    pred = _abi.RowPredicate(0, 0, 0, 0, deny)
    all_ids = np.arange(rows, dtype=np.uint64)
    rng = np.random.default_rng(16)

    def filtered_loop():     # straight through ctypes on preallocated arrays, like the baselines of the unfiltered mode
        for j in range(n_stores):
            assert L.wax_hip_search_predicate(hs[j], qp[j], dims, k, 0, None, 0, 0, 0.0, ctypes.byref(pred), ip[j], sp[j], k, ctypes.byref(got)) == 0
            a_counts[j] = got.value

    def many_filtered():
        return wax.searchManyFiltered(engines, queries, k, denyFlags=deny)

    def many():
        return wax.searchMany(engines, queries, k)

    for case in ("random_sixteenth", "contiguous_quarter"):
        for e in engines:
            fl = np.zeros(rows, np.uint32)
            if case == "random_sixteenth":
                fl[rng.random(rows) < 1.0 / 16] = 1
            else:
                r0 = int(rng.integers(0, rows - rows // 4))
                fl[r0:r0 + rows // 4] = 1
            e.setAttributes(all_ids, None, fl)
        masked0 = sum(e.getTuning("search_many_masked") for e in engines)
        ids, scores, counts = many_filtered()
        a_ids[:] = 0
        a_scores[:] = 0
        filtered_loop()      # (b) returns what (a) returns
        assert np.array_equal(counts, a_counts) and (counts == k).all() and np.array_equal(ids[:, :k], a_ids) and np.array_equal(scores[:, :k], a_scores), case
        masked = sum(e.getTuning("search_many_masked") for e in engines) - masked0
        forms = {"filtered_loop_ms": filtered_loop, "many_filtered_ms": many_filtered, "many_ms": many}
        for f in forms.values():
            f()
        t = {name: [] for name in forms}
        for _ in range(args.reps):
            for name, f in forms.items():
                t[name].append(timed(f))
        row = {"case": case, "store_bytes_total": rows * dims * 4 * n_stores, "masked_pairs_of_first_call": masked}
        row.update({name: round(statistics.median(v), 4) for name, v in t.items()})
        row["filtered_loop_over_many_filtered"] = round(row["filtered_loop_ms"] / row["many_filtered_ms"], 3)      # a / b
        row["many_filtered_over_filtered_loop"] = round(row["many_filtered_ms"] / row["filtered_loop_ms"], 3)      # b / a
        row["many_filtered_over_many"] = round(row["many_filtered_ms"] / row["many_ms"], 3)                        # b / c
        res["cases"].append(row)
        print(json.dumps(row), flush=True)
    for e in engines:
        e.close()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if args.predicate:
    predicate_mode()
    sys.exit(0)

out = {"dims": dims, "topk": k, "stores": n_stores, "reps": args.reps, "depth": args.depth, "table": []}
for rows in [int(x) for x in args.rows.split(",")]:
    engines = build_stores(rows)

    # (a) and (b) call the C entry points straight through ctypes on preallocated arrays (a microsecond or two of Python per call), so
    # that the baselines are the library's per-call cost, not the wrapper's
    L = engines[0]._lib
    f32, u32, u64 = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
    a_ids, a_scores = np.zeros((n_stores, k), np.uint64), np.zeros((n_stores, k), np.float32)
    got = ctypes.c_uint32(0)
    hs = [e._h for e in engines]
    qp = [queries[j].ctypes.data_as(f32) for j in range(n_stores)]
    ip = [a_ids[j].ctypes.data_as(u64) for j in range(n_stores)]
    sp = [a_scores[j].ctypes.data_as(f32) for j in range(n_stores)]

    def loop():
        for j in range(n_stores):
            assert L.wax_hip_search(hs[j], qp[j], dims, k, ip[j], sp[j], k, ctypes.byref(got)) == 0

    def pipelined():
        tickets = [ctypes.c_uint64(0) for _ in range(n_stores)]
        done = 0
        for j in range(n_stores):
            if j - done == args.depth:
                assert L.wax_hip_search_collect(hs[done], tickets[done], ip[done], sp[done], k, ctypes.byref(got)) == 0
                done += 1
            assert L.wax_hip_search_submit(hs[j], qp[j], dims, k, ctypes.byref(tickets[j])) == 0
        while done < n_stores:
            assert L.wax_hip_search_collect(hs[done], tickets[done], ip[done], sp[done], k, ctypes.byref(got)) == 0
            done += 1

    def many():
        return wax.searchMany(engines, queries, k)

    ids, scores, counts = many()
    for fn in (loop, pipelined):     # (c) returns what (a) and (b) return
        a_ids[:] = 0
        a_scores[:] = 0
        fn()
        assert (counts == k).all() and np.array_equal(ids[:, :k], a_ids) and np.array_equal(scores[:, :k], a_scores), fn.__name__
    pooled = sum(e.getTuning("search_many_pooled") for e in engines)
    forms = {"loop_ms": loop, "pipelined_ms": pipelined, "many_ms": many}
    for f in forms.values():
        f()
    t = {name: [] for name in forms}
    for _ in range(args.reps):
        for name, f in forms.items():
            t[name].append(timed(f))
    row = {"rows": rows, "store_bytes_total": rows * dims * 4 * n_stores, "pooled_pairs_of_first_call": pooled}
    row.update({name: round(statistics.median(v), 4) for name, v in t.items()})
    row["pipelined_over_many"] = round(row["pipelined_ms"] / row["many_ms"], 3)
    row["loop_over_many"] = round(row["loop_ms"] / row["many_ms"], 3)
    row["many_gb_per_s"] = round(row["store_bytes_total"] / row["many_ms"] / 1e6, 1)
    out["table"].append(row)
    print(json.dumps(row), flush=True)
    for e in engines:
        e.close()
    del engines
    torch.cuda.empty_cache()
# the default of "search_many_max_rows": the largest measured size at which (c) is at least 1.10 x faster than (b) per pair
wins = [r["rows"] for r in out["table"] if r["pipelined_over_many"] >= 1.10]
out["largest_rows_with_10_percent_win"] = max(wins) if wins else None
print(json.dumps(out))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
