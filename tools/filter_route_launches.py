#!/usr/bin/env python3
"""The kernels each route of the single-query filtered / predicate search launches, in order, and those of one batched predicate
call.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/filter_route_launches.py
    python tools/filter_route_launches.py --trace DIR/.../*_kernel_trace.csv > launches.txt

Without --trace: a 4 099 x 384 cosine store with attributes, every route warmed once (workspaces, id table, attribute columns),
then ONE call per route with a one-list rank fusion between two calls — its kernel is the separator in the trace. The last call is
the batched one: 256 queries, 16 distinct time windows of 1/16 of the rows, 16 queries each, no allow-list.
With --trace: the dispatches of that run's kernel trace in start order, cut at the separators: one `name grid` line per launch
under the route's title. Two builds launch the same sequence when their outputs are equal."""
import argparse
import csv
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B_HALF = 1 << 8
# title -> (allow-list or None, deny bits, predicate_route, top_k)
CALLS = [
    ("allow-list, short (host staging, gather tail)", "short", 0, 0, 10),
    ("allow-list, long (probe with sums, emit, gather tail)", "long", 0, 0, 10),
    ("predicate, gather route", None, B_HALF, 1, 10),
    ("predicate, masked scan, k 10 (merge alone)", None, B_HALF, 2, 10),
    ("predicate, masked scan, k 65 (short selection, gated merge)", None, B_HALF, 2, 65),
    ("predicate and short list (host staging, gather tail)", "short", B_HALF, 1, 10),
    ("predicate and long list, gather route", "long", B_HALF, 1, 10),
    ("predicate and long list, masked scan", "long", B_HALF, 2, 10),
]
BATCH_TITLE = "batched predicates: 16 windows x 16 queries, no list (three row-list launches, one gather, one merge)"


def run():
    import oracle
    import wax_amd as wax
    from wax_amd.hybrid_search import rrfFusionArrays
    n, dims = 4_099, 384
    rng = np.random.default_rng(0)
    ids = np.arange(n, dtype=np.uint64) * 3 + 7
    eng = wax.HIPVectorEngine(dimensions=dims)
    eng.addBatch(ids, np.ascontiguousarray(oracle.gaussian_unit_rows(0, n, dims), dtype=np.float32))
    eng.setAttributes(ids, np.arange(n, dtype=np.int64), np.where(rng.random(n) < 0.5, B_HALF, 0).astype(np.uint32))
    lists = {"short": ids[rng.choice(n, 300, replace=False)], "long": ids[rng.choice(n, 4_096, replace=False)]}
    q = oracle.gaussian_unit_queries(1, dims)[0]

    def call(allow, deny, route, k):
        eng.setTuning("predicate_route", route)
        got = eng.searchFiltered(q, k, frameIds=None if allow is None else lists[allow], denyFlags=deny)
        assert len(got[0]) == k

    for _, allow, deny, route, k in CALLS:
        call(allow, deny, route, k)
    for _, allow, deny, route, k in CALLS:
        rrfFusionArrays([(1.0, [1, 2, 3])])
        call(allow, deny, route, k)
    eng.setTuning("predicate_route", 0)
    qs = oracle.gaussian_unit_queries(256, dims)
    windows = [(j * (n - n // 16) // 16 + 1, j * (n - n // 16) // 16 + 1 + n // 16) for j in range(16)]

    def batched():
        before = eng.getTuning("predicate_batch_queries")
        _, _, counts = eng.searchBatchFiltered(qs, 10, timeRange=[windows[q // 16] for q in range(256)])
        assert (counts == 10).all() and eng.getTuning("predicate_batch_queries") - before == 256

    batched()
    rrfFusionArrays([(1.0, [1, 2, 3])])
    batched()
    eng.close()


def report(path):
    with open(path) as fh:
        rows = list(csv.DictReader(fh))
    assert rows and {"Kernel_Name", "Start_Timestamp"} <= set(rows[0]), f"not a rocprofv3 kernel trace: columns {sorted(rows[0]) if rows else []}"
    # start order is launch order here: every call ends with a synchronisation, so no two calls' kernels overlap
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    calls, cur = [], None
    for r in rows:
        name = r["Kernel_Name"]
        if "rrf_fuse_kernel" in name:
            cur = []
            calls.append(cur)
        elif cur is not None:
            grid = [r.get(f"Grid_Size_{a}") for a in "XYZ"]
            cur.append(f"{name}  grid {r.get('Grid_Size') or 'x'.join(g for g in grid if g)}")
    titles = [c[0] for c in CALLS] + [BATCH_TITLE]
    assert len(calls) == len(titles), f"{len(calls)} separators in the trace for {len(titles)} calls"
    assert all(calls), "a call without a single kernel: the separators do not bracket the calls"
    for title, launches in zip(titles, calls):
        print(f"## {title}")
        for ln in launches:
            print(ln)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--trace", default=None, help="a kernel_trace.csv of this script's run: print the launches per call")
    args = ap.parse_args()
    if args.trace:
        report(args.trace)
    else:
        run()
