#!/usr/bin/env python3
"""Record what setTuning / getTuning do, key by key, as tests/golden/tuning_registry.json holds it (tests/test_tuning_table_gpu.py
replays the record against the tree under test). Only the public Python API and _abi.last_error() are used, so the same script
runs against any build of the ABI (WAX_HIP_LIB names another libwaxhip.so).

  keys   --tuning tuning.inc --sharded sharded.inc --out keys.json   the key names of a source tree: the rows of its tuning table,
                                                                    or its `k == "name"` chains if it is older (no GPU)
  record --keys keys.json --out rec.json                            part A and part B in this process (MI355X)
  merge  rec1.json rec2.json rec3.json --out tuning_registry.json   part A must agree; a part-B key whose records disagree
                                                                    is stored with its values under "unstable"

Part A: every settable key on a 64-d engine and on a devices=[0, 0] handle ("shard_min_mb" 0): the value a fresh engine reports,
then for each probe value the return class, the error text and what getTuning reports afterwards. No search runs.
Part B: every readable key after workload() on one 384-d cosine engine of 4 096 rows and on a devices=[0, 0, 0] handle.
"""
import argparse
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PROBES = [-2**63, -2**31 - 1, -2, -1, 0, 1, 2, 3, 4, 5, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 192, 256, 1000, 1001,
          1002, 1024, 1025, 2047, 2048, 2049, 2176, 4095, 4096, 4097, 16384, 65536, 69632, 86016, 86017, 2**20, 2**20 + 1,
          2**31 - 1, 2**31, 2**32 - 1, 2**32, 2**63 - 1]
UNKNOWN_KEY = "no_such_key"
WRONG_CASE_KEY = "Scan_Mirror"
NEVER_COMPARED = ("store_ptr",)          # an address


def probes_for(key):
    if key == "batch_prof_ptr":          # any other value is a device address
        return [0]
    if key == "exchange":                # 1 loads RCCL and builds communicators
        return [v for v in PROBES if v != 1]
    return PROBES


def source_keys(tuning_path, sharded_path):
    """Key names of a source tree: from the rows of the tuning table (`{"name", how to set, how to get, what a handle answers}`, one
    per line) and the handle's own branches in sharded.inc, or, for a tree from before the table, from its four `k == "name"` chains.
    "sharded_readable" is what a handle answers itself: its own keys and the ones it sums."""
    def names(text, start, end):
        i = text.index(start)
        return sorted(set(re.findall(r'k == "([a-z_0-9]+)"', text[i:text.index(end, i)])))
    src = open(tuning_path).read()
    sh = open(sharded_path).read()
    rows = re.findall(r'^ *\{"([a-z_0-9]+)",(.*)$', src, re.M)
    if rows:
        summed = {n for n, rest in rows if re.search(r"SUM_SHARDS\},", rest)}
        return {"settable": sorted(n for n, rest in rows if "not_set()" not in rest),
                "readable": sorted(n for n, rest in rows if "not_get()" not in rest),
                "sharded_settable": names(sh, "int sh_set_tuning(", "sh_get_tuning("),
                "sharded_readable": sorted(summed | set(names(sh, "int64_t sh_get_tuning(", "void sh_destroy(")))}
    return {"settable": names(src, "int wax_hip_set_tuning(", "wax_hip_get_tuning("),
            "readable": names(src, "int64_t wax_hip_get_tuning(", "int wax_hip_time_scan_kernel("),
            "sharded_settable": names(sh, "int sh_set_tuning(", "sh_get_tuning("),
            "sharded_readable": names(sh, "int64_t sh_get_tuning(", "void sh_destroy(")}


def _set(eng, key, value):
    """-> [exception class or "ok", error text]"""
    from wax_amd import _abi
    try:
        eng.setTuning(key, value)
        return ["ok", ""]
    except Exception as exc:   # noqa: BLE001 — the class is the record
        return [type(exc).__name__, _abi.last_error()]


def probe_keys(eng, keys):
    fresh = {k: eng.getTuning(k) for k in keys}
    out = {}
    for k in keys:
        out[k] = {"fresh": fresh[k], "probes": [[v] + _set(eng, k, v) + [eng.getTuning(k)] for v in probes_for(k)]}
    return out


def part_a(wax, keys):
    single = sorted(keys["settable"])
    sharded = sorted(set(keys["settable"]) | set(keys["sharded_settable"]))
    out = {}
    with wax.HIPVectorEngine(metric=wax.VectorMetric.cosine, dimensions=64, device=0) as eng:
        out["single"] = probe_keys(eng, single)
        out["unknown"] = {"set": _set(eng, UNKNOWN_KEY, 1), "get": eng.getTuning(UNKNOWN_KEY)}
        out["wrong_case"] = {"set": _set(eng, WRONG_CASE_KEY, 1), "get": eng.getTuning(WRONG_CASE_KEY)}
    with wax.HIPVectorEngine(metric=wax.VectorMetric.cosine, dimensions=64, devices=[0, 0]) as eng:
        eng.setTuning("shard_min_mb", 0)
        out["sharded"] = probe_keys(eng, sharded)
        out["sharded_unknown"] = {"set": _set(eng, UNKNOWN_KEY, 1), "get": eng.getTuning(UNKNOWN_KEY)}
    return out


def workload(wax, eng, sharded):
    """The fixed workload of part B: every call blocks, except the "mirror_share" 2 submissions that make a shared pass, two at a time.
    The counts of the calls are chosen so that counters of one family end at different values (a row wired to its neighbour shows)."""
    import numpy as np
    n, dims = 4096, 384
    rng = np.random.default_rng(23)
    rows = rng.standard_normal((n, dims)).astype(np.float32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    qs = rng.standard_normal((64, dims)).astype(np.float32)
    qs /= np.linalg.norm(qs, axis=1, keepdims=True)
    ids = np.arange(n, dtype=np.uint64) + 1000
    if sharded:
        eng.setTuning("shard_min_mb", 0)
    eng.setTuning("scan_mirror", 2)
    eng.addBatch(ids, rows)
    eng.setTuning("mirror_bits", 16)
    eng.searchArrays(qs[0], 10)
    eng.setTuning("mirror_bits", 8)
    for i in (1, 2, 35, 36, 41, 42, 43):                 # the third 8-bit query in a row builds the code mirror: five passes over it
        eng.searchArrays(qs[i], 10)
    # one row overwritten (the first shard's) and seven appended, then a bf16 query and no 8-bit one: the bf16 mirror converts a second
    # time and the code mirror does not, which tells "mirror_conversions" / "mirror_rows_converted" from their 8-bit twins
    eng.addBatch(np.concatenate([ids[:1], np.arange(7, dtype=np.uint64) + 100000]), qs[51:59])
    eng.setTuning("mirror_bits", 16)
    eng.searchArrays(qs[40], 10)
    eng.setTuning("mirror_bits", 0)
    eng.searchArrays(qs[3], 300)
    eng.setTuning("force_general", 1)
    eng.searchArrays(qs[4], 10)
    eng.setTuning("force_general", 0)
    eng.setTuning("scan_mirror", 0)                      # one query on the f32 scan
    eng.searchArrays(qs[5], 10)
    eng.searchArrays(qs[37], 300)
    eng.setTuning("done_flag", 0)                        # ... one that waits on an event, two with the query uploaded
    eng.searchArrays(qs[59], 10)
    eng.setTuning("done_flag", 1)
    eng.setTuning("query_args", 0)
    eng.searchArrays(qs[60], 10)
    eng.searchArrays(qs[61], 10)
    eng.setTuning("query_args", 1)
    eng.setTuning("scan_mirror", 2)
    eng.setTuning("mirror_share", 2)                     # two submissions in flight: one shared pass
    for pair in ((6, 7), (44, 45), (62, 63)):
        tickets = [eng.submit(qs[i], 10) for i in pair]
        for t in tickets:
            eng.collect(t, 10)
    eng.setTuning("mirror_share", 1)
    eng.searchBatch(qs[:32], 10)
    eng.setTuning("batch_mode", 0)                       # a batch the MFMA pipelines do not take: shared exact passes
    eng.searchBatch(qs[:17], 10)
    eng.setTuning("batch_mode", 1)
    eng.setTuning("batch_onepass", 0)                    # a batch on the slab pipeline
    eng.searchBatch(qs[:18], 10)
    eng.setTuning("batch_onepass", 1)
    eng.searchFiltered(qs[8], 10, frameIds=ids[:50])
    eng.searchFiltered(qs[9], 10, frameIds=ids)          # a list long enough to be resolved on the device
    eng.setAttributes(ids, timestamps=np.arange(n, dtype=np.int64), flags=((np.arange(n) % 4 == 0).astype(np.uint32) << 8))
    window = (1000, 3000)
    eng.searchFiltered(qs[10], 10, timeRange=window, denyFlags=0x100)            # auto route
    eng.setTuning("predicate_route", 1)
    eng.searchFiltered(qs[11], 10, timeRange=window)
    eng.searchFiltered(qs[12], 10, frameIds=ids[:2000], timeRange=window)
    eng.searchFiltered(qs[46], 10, timeRange=window, denyFlags=0x100)
    eng.searchFiltered(qs[48], 10, timeRange=(0, 500))
    eng.searchFiltered(qs[47], 10, timeRange=(0, 500))
    eng.setTuning("predicate_route", 2)
    for i in (13, 14, 15):
        eng.searchFiltered(qs[i], 10, timeRange=window, denyFlags=0x100)
    eng.setAttributes(ids[4000:4010], flags=np.full(10, 0x200, dtype=np.uint32))   # the device columns are uploaded again from row 4000
    eng.setTuning("predicate_mirror", 2)
    for i in (16, 17, 18, 19, 49, 50, 39):
        eng.searchFiltered(qs[i], 10, timeRange=window)
    eng.setTuning("predicate_mirror", 1)
    eng.setTuning("predicate_route", 0)
    lists = [ids[:100], ids[50:400], None, ids[1000:1010]]
    eng.searchBatchFiltered(qs[20:24], 10, frameIds=lists)
    eng.searchBatchFiltered(qs[24:29], 10, frameIds=lists + lists[:1], timeRange=[window, None, (0, 2000), window, window],
                            denyFlags=[0x100, 0, 0, 0, 0x100])   # the first and the last query share one (list, predicate) entry
    if not sharded:                                      # (searchMany takes single-device engines only)
        wax.searchManyFiltered([eng, eng], qs[38:40], 10, timeRange=window)
        wax.searchMany([eng, eng, eng], qs[30:33], 10)
        eng.setTuning("search_many", 0)
        wax.searchMany([eng], qs[33:34], 10)
        eng.setTuning("search_many", 1)
    assert eng.removeBatch(ids[5:15]) == 10
    eng.searchArrays(qs[34], 10)


def part_b(wax, keys):
    single = sorted(set(keys["readable"]) - set(NEVER_COMPARED))
    sharded = sorted((set(keys["readable"]) | set(keys["sharded_readable"])) - set(NEVER_COMPARED))
    out = {}
    with wax.HIPVectorEngine(metric=wax.VectorMetric.cosine, dimensions=384, device=0) as eng:
        workload(wax, eng, False)
        out["single"] = {k: eng.getTuning(k) for k in single}
    with wax.HIPVectorEngine(metric=wax.VectorMetric.cosine, dimensions=384, devices=[0, 0, 0]) as eng:
        workload(wax, eng, True)
        out["sharded"] = {k: eng.getTuning(k) for k in sharded}
    return out


def merge(records):
    a = records[0]["part_a"]
    for r in records[1:]:
        assert r["part_a"] == a, "part A differs between two records of one build"
        assert r["keys"] == records[0]["keys"]
    b, unstable = {}, {}
    for side in ("single", "sharded"):
        b[side], unstable[side] = {}, {}
        for k in records[0]["part_b"][side]:
            vals = [r["part_b"][side][k] for r in records]
            if all(v == vals[0] for v in vals):
                b[side][k] = vals[0]
            else:
                unstable[side][k] = vals
    return {"keys": records[0]["keys"], "part_a": a, "part_b": b, "unstable": unstable}


def dumps(obj, depth=3):
    """JSON with one line per key down to `depth` levels, compact below (a probe list stays one line)."""
    if depth == 0 or not isinstance(obj, dict) or not obj:
        return json.dumps(obj, sort_keys=True, separators=(",", ":"))
    return "{\n" + ",\n".join(json.dumps(k) + ":" + dumps(obj[k], depth - 1) for k in sorted(obj)) + "\n}" + ("\n" if depth == 3 else "")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("keys")
    p.add_argument("--tuning", required=True)
    p.add_argument("--sharded", required=True)
    p.add_argument("--out", required=True)
    p = sub.add_parser("record")
    p.add_argument("--keys", required=True)
    p.add_argument("--out", required=True)
    p = sub.add_parser("merge")
    p.add_argument("records", nargs="+")
    p.add_argument("--out", required=True)
    args = ap.parse_args()
    if args.cmd == "keys":
        result = source_keys(args.tuning, args.sharded)
    elif args.cmd == "record":
        import wax_amd
        keys = json.load(open(args.keys))
        result = {"keys": keys, "part_a": part_a(wax_amd, keys), "part_b": part_b(wax_amd, keys)}
    else:
        result = merge([json.load(open(r)) for r in args.records])
    with open(args.out, "w") as f:
        f.write(dumps(result))
    print(f"[tuning_snapshot] {args.cmd}: wrote {args.out}")


if __name__ == "__main__":
    main()
