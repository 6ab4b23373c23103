"""CPU tests of the host side: the C-ABI library loads and exports everything the header
declares, fails loudly without a GPU, and the pure-host logic (error mapping, VectorMath,
VectorSerializer header codec, hit decoding, shard bounds, host merge) is correct.
No compute entry point is exercised here."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import oracle
import helpers
from helpers import load_golden

REF = load_golden("reference_cases.json")


def test_library_exports_every_declared_symbol(hip_lib):
    from wax_amd import _abi
    declared = _abi.declared_symbols()
    assert len(declared) >= 30
    assert set(declared) == set(_abi.SIGNATURES), (set(declared) ^ set(_abi.SIGNATURES))
    for name in declared:
        assert hasattr(hip_lib, name), f"libwaxhip.so does not export {name}"
    assert hip_lib.wax_hip_abi_version() == 2


def test_mirror8_snapshot_entry_is_declared_bound_and_refuses_a_null_engine(hip_lib):
    """The code mirror's diagnostic read-out: exported, declared in the header and in _abi.py with the header's argument list, the
    ABI version unchanged by it, and a NULL engine (or a NULL word pointer) refused with a message before any device is touched."""
    from wax_amd import _abi
    name = "wax_hip_mirror8_snapshot"
    assert name in _abi.declared_symbols() and hasattr(hip_lib, name)
    text = " ".join(open(_abi.HEADER_PATH).read().split())
    assert ("int wax_hip_mirror8_snapshot(wax_hip_engine* e, uint64_t first_row, uint64_t n_rows, uint8_t* out_codes, float* out_meta, "
            "float* out_max_norm, uint64_t* out_rows_coded);") in text
    restype, argtypes = _abi.SIGNATURES[name]
    assert restype is ctypes.c_int and argtypes == [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint8),
                                                    ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float),
                                                    ctypes.POINTER(ctypes.c_uint64)]
    assert "#define WAX_HIP_ABI_VERSION 2\n" in open(_abi.HEADER_PATH).read() and hip_lib.wax_hip_abi_version() == 2
    max_norm, rows = ctypes.c_float(-1.0), ctypes.c_uint64(77)
    rc = hip_lib.wax_hip_mirror8_snapshot(None, 0, 0, None, None, ctypes.byref(max_norm), ctypes.byref(rows))
    assert rc == _abi.ERR_INVALID_ARGUMENT and "null" in _abi.last_error()
    assert max_norm.value == -1.0 and rows.value == 77


def test_library_is_a_gfx950_code_object():
    from wax_amd import build
    path = build.build()
    out = subprocess.run(["strings", "-n", "6", path], capture_output=True, text=True).stdout
    assert "gfx950" in out
    assert "scan_kernel" in out


def test_header_has_no_torch_or_hip_types():
    from wax_amd import _abi
    text = open(_abi.HEADER_PATH).read()
    code = "\n".join(l for l in text.splitlines() if not l.strip().startswith(("*", "/*", "//")))
    for banned in ("torch", "at::", "hipStream_t", "hipError_t", "std::"):
        assert banned not in code


def test_no_device_fails_loudly(hip_lib):
    """On a box without a gfx950 GPU every engine call errors; nothing silently falls back."""
    from wax_amd import HIPVectorEngine, InvalidToc, VectorMetric
    if hip_lib.wax_hip_available():
        pytest.skip("GPU present")
    assert HIPVectorEngine.isAvailable() is False
    with pytest.raises(InvalidToc) as ei:
        HIPVectorEngine(metric=VectorMetric.cosine, dimensions=384)
    assert "not available" in str(ei.value)


def test_product_never_imports_oracle():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for dirpath, _, files in os.walk(os.path.join(root, "wax_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".hpp", ".cpp")):
                text = open(os.path.join(dirpath, f), errors="replace").read()
                assert "import oracle" not in text and "from oracle" not in text, f
                assert "wax_oracle" not in text, f


def test_every_settable_tuning_key_is_documented_in_the_header():
    """The boundary is include/wax_hip.h: a key wax_hip_set_tuning accepts (single-device engine or sharded handle) that the header's
    tunables block does not name is an undocumented switch behind the shipping ABI. The keys of an engine are the rows of the table in
    tuning.inc (one line each, `{"name", how to set, how to get, what a sharded handle answers}`), the handle's own are the branches of
    sh_set_tuning; both sets, and the rows a handle sums, are the ones tests/golden/tuning_registry.json recorded."""
    import json
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "wax_amd", "csrc", "tuning.inc")).read()       # (engine.hip's translation unit, cut into files in round 6)
    rows = re.findall(r'^ *\{"([a-z_0-9]+)",(.*)$', src, re.M)
    names = [name for name, _ in rows]
    assert len(names) == len(set(names)), sorted(n for n in set(names) if names.count(n) > 1)
    settable = {name for name, rest in rows if "not_set()" not in rest}
    readable = {name for name, rest in rows if "not_get()" not in rest}
    summed = {name for name, rest in rows if re.search(r"SUM_SHARDS\},", rest)}
    assert all(re.search(r"(FIRST_SHARD|SUM_SHARDS)\},", rest) for _, rest in rows)
    sh = open(os.path.join(root, "wax_amd", "csrc", "sharded.inc")).read()
    i = sh.index("int sh_set_tuning(")
    handle = set(re.findall(r'k == "([a-z_0-9]+)"', sh[i:sh.index("sh_get_tuning(", i)]))
    keys = settable | handle
    documented = set(re.findall(r'"([a-z_0-9]+)"', open(os.path.join(root, "include", "wax_hip.h")).read()))
    assert len(keys) > 30 and {"time_kernels", "merge_overlap_mb", "batch_qfrag", "exchange", "shard_min_mb"} <= keys
    assert keys <= documented, sorted(keys - documented)
    recorded = json.load(open(os.path.join(root, "tests", "golden", "tuning_registry.json")))["keys"]
    assert sorted(settable) == recorded["settable"], sorted(settable ^ set(recorded["settable"]))
    assert sorted(readable) == recorded["readable"], sorted(readable ^ set(recorded["readable"]))
    assert sorted(handle) == recorded["sharded_settable"], sorted(handle ^ set(recorded["sharded_settable"]))
    # what the handle summed when the record was made: the names of its own condition that are keys of an engine
    assert summed == set(recorded["sharded_readable"]) & set(recorded["readable"]), sorted(summed ^ (set(recorded["sharded_readable"]) & set(recorded["readable"])))


def test_create_argument_validation(hip_lib):
    from wax_amd import _abi
    h = ctypes.c_void_p()
    assert hip_lib.wax_hip_engine_create(0, 0, -1, ctypes.byref(h)) == _abi.ERR_INVALID_ARGUMENT
    assert "dimensions must be > 0" in _abi.last_error()  # MetalVectorEngine.swift:155
    assert hip_lib.wax_hip_engine_create(0, 1000001, -1, ctypes.byref(h)) == _abi.ERR_CAPACITY
    assert hip_lib.wax_hip_engine_create(7, 4, -1, ctypes.byref(h)) == _abi.ERR_METRIC_UNSUPPORTED
    assert not h.value


def test_error_mapping():
    from wax_amd import _abi, errors
    assert issubclass(errors.EncodingError, errors.WaxError)
    _abi.lib()
    for code, exc in [(_abi.ERR_DIM_MISMATCH, errors.EncodingError), (_abi.ERR_CAPACITY, errors.CapacityExceeded),
                      (_abi.ERR_NO_DEVICE, errors.InvalidToc), (_abi.ERR_BAD_SEGMENT, errors.InvalidToc),
                      (_abi.ERR_ALLOC, errors.InvalidToc)]:
        with pytest.raises(exc):
            errors.raise_for_status(code)
    errors.raise_for_status(0)


def test_vector_metric_and_clamp():
    from wax_amd import VectorMetric, clampTopK
    c = REF["constants"]
    assert {m.name: int(m) for m in VectorMetric} == c["similarity_raw"]
    assert clampTopK(0) == 1 and clampTopK(-3) == 1 and clampTopK(10 ** 9) == c["max_results"] and clampTopK(30) == 30
    for m in VectorMetric:
        for d in (0.0, 0.25, 1.5, float("inf"), float("nan")):
            assert m.score(d) == pytest.approx(oracle.score_from_distance(int(m), d))


def test_vector_math_matches_reference_cases():
    from wax_amd import VectorMath
    for c in REF["vector_math"]:
        assert VectorMath.isNormalizedL2(c["vector"]) == c["isNormalizedL2"]
    v = np.array([3.0, 4.0], dtype=np.float32)
    assert np.allclose(VectorMath.normalizeL2(v), [0.6, 0.8])
    assert np.array_equal(VectorMath.normalizeL2(np.zeros(3, np.float32)), np.zeros(3, np.float32))
    assert VectorMath.isNormalizedL2([]) is False
    r = oracle.gaussian_unit_queries(4, 384) * np.float32(3.0)
    for q in r:
        assert np.allclose(VectorMath.normalizeL2(q), oracle.normalize_l2(q), atol=1e-7)


def test_vector_serializer_header_codec():
    from wax_amd import InvalidToc, VectorSerializer
    vec = oracle.gaussian_unit_rows(0, 3, 4)
    ids = np.array([5, 6, 7], dtype=np.uint64)
    blob = oracle.mv2v_serialize(0, vec, ids)
    assert VectorSerializer.detectEncoding(blob) == VectorSerializer.VecEncoding.metal
    kind, info, v2, i2 = VectorSerializer.decodeVecSegment(blob)
    assert kind == "metal" and info.dimension == 4 and info.vectorCount == 3 and info.payloadLength == 48
    assert np.array_equal(v2, vec) and np.array_equal(i2, ids)
    us = b"MV2V" + struct.pack("<HBBIQQ", 1, 1, 0, 4, 3, 5) + b"\x00" * 8 + b"hello"
    assert VectorSerializer.detectEncoding(us) == VectorSerializer.VecEncoding.uSearch
    assert VectorSerializer.decodeVecSegment(us)[0] == "uSearch"
    for bad in (blob[:5], b"NOPE" + blob[4:], blob + b"x", blob[:6] + b"\x09" + blob[7:]):
        with pytest.raises(InvalidToc):
            VectorSerializer.decodeVecSegment(bad) if len(bad) >= 8 else VectorSerializer.detectEncoding(bad)


def test_hits_to_results_host_tail(hip_lib):
    """The host tail of search (MetalVectorEngine.swift:592-611): padding and non-finite dropped,
    distance -> score, key decoding is the inverse of the device encoding."""
    from wax_amd import HIPVectorEngine, VectorMetric, _abi

    def key(d, row):
        b = struct.unpack("<i", struct.pack("<f", d))[0]
        o = b ^ ((b >> 31) & 0x7FFFFFFF)
        return (o << 32) | row

    hits = np.array([[key(0.25, 3), 103], [key(0.5, 1), 101], [key(float("inf"), 9), 109],
                     [_abi.KEY_PAD, -1], [key(-0.5, 2), 102]], dtype=np.int64)
    ids, scores = HIPVectorEngine.hitsToResults(VectorMetric.cosine, hits)
    assert list(ids) == [103, 101, 102]
    assert np.allclose(scores, [0.75, 0.5, 1.5])
    ids, scores = HIPVectorEngine.hitsToResults(VectorMetric.l2, hits[:2])
    assert np.allclose(scores, [-0.25, -0.5])
    # signed key order == (distance asc, row asc), negatives and -0 included
    ds = [-2.0, -0.0, 0.0, 1e-30, 0.5, 0.5, 3.0, float("inf")]
    keys = [key(d, r) for r, d in enumerate(ds)]
    assert keys == sorted(keys)


def test_shard_bounds_and_host_merge():
    from wax_amd import sharded
    n = 10_000_000
    for world in (1, 2, 4, 8, 3):
        spans = [sharded.shard_bounds(n, world, r) for r in range(world)]
        assert spans[0][0] == 0 and spans[-1][1] == n
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    assert sharded.shard_bounds(10, 4, 3) == (9, 10)
    assert sharded.shard_bounds(10, 8, 7) == (10, 10)  # empty tail shard
    g = np.array([[5, 50], [1, 10], [sharded.KEY_PAD, -1], [3, 30], [2, 20]], dtype=np.int64)
    m = sharded.merge_hits_host(g, 3)
    assert m[:, 0].tolist() == [1, 2, 3] and m[:, 1].tolist() == [10, 20, 30]
    m = sharded.merge_hits_host(g[:2], 4)
    assert m[:, 0].tolist() == [1, 5, sharded.KEY_PAD, sharded.KEY_PAD]


def test_decode_hits_matches_c_host_tail_and_batch_merge(hip_lib):
    from wax_amd import HIPVectorEngine, VectorMetric, _abi, sharded

    def key(d, row):
        b = struct.unpack("<i", struct.pack("<f", d))[0]
        return ((b ^ ((b >> 31) & 0x7FFFFFFF)) << 32) | row

    rng = np.random.default_rng(3)
    nq, k = 5, 6
    hits = np.empty((nq, k, 2), dtype=np.int64)
    for q in range(nq):
        ds = np.sort(rng.standard_normal(k).astype(np.float32))
        for i in range(k):
            hits[q, i] = (key(float(ds[i]), 10 * q + i), 1000 + 10 * q + i)
    hits[1, 4:] = (_abi.KEY_PAD, -1)
    hits[2, 5] = (key(float("inf"), 77), 1077)
    for metric in (VectorMetric.cosine, VectorMetric.dot, VectorMetric.l2):
        ids, scores, valid = sharded.decode_hits(metric, hits)
        for q in range(nq):
            c_ids, c_scores = HIPVectorEngine.hitsToResults(metric, hits[q])
            assert list(ids[q][valid[q]]) == list(c_ids)
            assert np.array_equal(scores[q][valid[q]], c_scores)
    # per-query merge over shards == global sort by key
    world = 3
    g = np.empty((world, nq, k, 2), dtype=np.int64)
    allkeys = rng.permutation(world * nq * k * 4)[:world * nq * k].reshape(world, nq, k).astype(np.int64)
    allkeys.sort(axis=2)
    g[..., 0] = allkeys
    g[..., 1] = allkeys + 5
    m = sharded.merge_batch_hits_host(g, k)
    for q in range(nq):
        exp = np.sort(allkeys[:, q, :].reshape(-1))[:k]
        assert np.array_equal(m[q, :, 0], exp) and np.array_equal(m[q, :, 1], exp + 5)


def _build_c_smoke(tmp_path):
    from wax_amd import build
    lib = build.build()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "c_abi_smoke")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(root, "include"),
                    os.path.join(root, "tests", "c_abi", "smoke.c"), "-L" + os.path.dirname(lib), "-lwaxhip",
                    "-Wl,-rpath," + os.path.dirname(lib), "-o", exe], check=True)
    return exe


def test_plain_c_consumer_links_and_fails_loudly_without_gpu(hip_lib, tmp_path):
    exe = _build_c_smoke(tmp_path)
    if hip_lib.wax_hip_available():
        pytest.skip("GPU present: covered by the gpu-marked twin")
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "no-device" in out.stdout


@pytest.mark.gpu
def test_plain_c_consumer_on_gpu(hip_lib, tmp_path):
    if hip_lib.wax_hip_device_count() == 0:
        pytest.skip("no HIP device on this host")
    exe = _build_c_smoke(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "c-abi ok: id 20" in out.stdout


def _run_hpp_consumer(tmp_path):
    """include/wax_hip.hpp (the C++17 convenience wrapper) is compiled and linked against libwaxhip by a real
    consumer; without a GPU the program checks the loud NO_DEVICE error through the wrapper's exception."""
    from wax_amd import build
    lib = build.build()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "hpp_consumer.cpp"
    src.write_text(r'''
#include <cstdio>
#include <cstring>
#include "wax_hip.hpp"
int main() {
    try {
        wax_hip::VectorEngine e(WAX_HIP_METRIC_COSINE, 4);
        e.add(1, {1.f, 0.f, 0.f, 0.f});
        e.addBatch({2, 3}, {0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f});
        auto hits = e.search({0.9f, 0.1f, 0.f, 0.f}, 2);
        if (hits.size() != 2 || hits[0].first != 1) return 5;
        std::vector<uint64_t> allow{2, 3};
        auto f = e.searchFiltered({0.9f, 0.1f, 0.f, 0.f}, 5, &allow, nullptr);
        if (f.size() != 2 || f[0].first != 2) return 6;
        auto blob = e.serialize();
        wax_hip::VectorEngine e2(WAX_HIP_METRIC_COSINE, 4);
        e2.deserialize(blob);
        if (e2.count() != 3 || e2.dimensions() != 4) return 7;
        e2.remove(2);
        if (e2.count() != 2) return 8;
        std::printf("hpp ok\n");
        return 0;
    } catch (const wax_hip::Error& err) {
        if (!wax_hip::VectorEngine::isAvailable() && err.status == WAX_HIP_ERR_NO_DEVICE && std::strlen(err.what()) > 0) {
            std::printf("no-device: %s\n", err.what());
            return 0;
        }
        std::printf("unexpected error %d: %s\n", err.status, err.what());
        return 9;
    }
}
''')
    exe = str(tmp_path / "hpp_consumer")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(root, "include"), str(src),
                    "-L" + os.path.dirname(lib), "-lwaxhip", "-Wl,-rpath," + os.path.dirname(lib), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


def test_cpp_wrapper_header_compiles_against_the_c_abi(hip_lib, tmp_path):
    out = _run_hpp_consumer(tmp_path)
    assert ("hpp ok" in out) if hip_lib.wax_hip_available() else ("no-device" in out)


@pytest.mark.gpu
def test_cpp_wrapper_on_gpu(hip_lib, tmp_path):
    if hip_lib.wax_hip_device_count() == 0:
        pytest.skip("no HIP device on this host")
    assert "hpp ok" in _run_hpp_consumer(tmp_path)


def test_sharded_create_validates_the_device_list(hip_lib):
    """wax_hip_engine_create_sharded fails loudly for an unavailable ordinal or an empty list (no GPU needed to see it)."""
    from wax_amd import _abi
    h = ctypes.c_void_p()
    n = hip_lib.wax_hip_device_count()
    devs = (ctypes.c_int * 2)(0, n + 7)
    assert hip_lib.wax_hip_engine_create_sharded(0, 384, devs, 2, ctypes.byref(h)) == _abi.ERR_NO_DEVICE
    assert f"HIP device {n + 7 if n else 0} not available" in _abi.last_error() and not h.value
    assert hip_lib.wax_hip_engine_create_sharded(0, 384, devs, 0, ctypes.byref(h)) == _abi.ERR_INVALID_ARGUMENT
    assert hip_lib.wax_hip_engine_create_sharded(0, 384, None, 2, ctypes.byref(h)) == _abi.ERR_INVALID_ARGUMENT
    assert hip_lib.wax_hip_shard_count(None) == 0


def test_bench_deterministic_embedder_rows_match_the_oracle():
    """bench.py's vectorised DeterministicEmbedder corpus (torch int64 arithmetic: FNV-1a over "doc-<i>", LCG, Float(Int64)
    / Float(Int64.max), L2 normalisation) against the oracle's C restatement of RAGBenchmarkSupport.swift:114-157, text
    by text — including every digit-count boundary."""
    import importlib.util
    import torch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("wax_bench", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    dims = 48
    for lo, hi in [(0, 12), (95, 105), (999, 1002), (123456, 123459), (999_998, 1_000_003), (9_999_999, 10_000_001)]:
        got = torch.cat([x for _, x in bench.deterministic_embedder_rows(torch, lo, hi, dims, torch.device("cpu"))]).numpy()
        assert got.shape == (hi - lo, dims)
        for i in range(lo, hi):
            exp = oracle.deterministic_embed(f"doc-{i}", dims, normalize=True)
            assert np.max(np.abs(got[i - lo] - exp)) <= 3e-7, (i, got[i - lo][:4], exp[:4])
            raw = oracle.deterministic_embed(f"doc-{i}", dims, normalize=False)
            assert np.allclose(got[i - lo] * np.linalg.norm(raw.astype(np.float64)), raw, atol=1e-6)


def _load_bench():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("wax_bench", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def _synthetic_full_record(bench, n_secondary, prose=1200):
    """A record shaped like bench.py's full output with every prose field at `prose` bytes — the shape that grew to 22 KB in
    round 3 and fell out of the driver's stdout tail."""
    blah = "x" * prose
    roof = {"bound": "hbm", "achieved": 6986.123456789, "peak": 8000.0, "unit": "GB/s", "frac": 0.873265432, "pipeline_achieved": 7064.9,
            "pipeline_frac": 0.8831123, "traffic": 15360180224.0, "traffic_source": blah, "kernel": "wax::scan_kernel (fused scan + per-wave top-k)",
            "kernel_avg_ms": 2.1987654321, "kernel_launches_timed": 60, "algorithmic_bytes_per_launch": 15360000000,
            "calibration": {"steps": 60, "ms_per_step": 2.21, "mode": blah}, "note": blah, "mfma_sustained_source": blah}
    sec = []
    for i in range(n_secondary):
        sec.append({"name": f"clustered_k100_{i}", "config": blah, "value": 1092655.338450946, "unit": "queries/s", "steps": 100, "warmup": 10,
                    "ms_per_step": 0.23429162974935025, "dtype": "bf16 GEMM, exact f32 re-score", "queries_per_step": 256,
                    "last_result_checksum": "0123456789abcdef", "roofline": dict(roof), "n_gpus": 8 if i % 2 else 1})
    sec.append({"name": "broken", "error": "RuntimeError: " + blah})
    return {
        "metric": "queries/sec, 10M x 384-dim f32 cosine top-10 brute-force scan (single query per step)", "value": 460.4123456789,
        "unit": "queries/s", "n_gpus": 8, "steps": 200, "warmup": 20, "ms_per_step": 2.17198765, "higher_is_better": True, "scaling": "strong",
        "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": blah, "workload_short": "10M x 384 f32 unit-Gaussian corpus in HBM, cosine top-10, 1 query/step", "rows": 10_000_000,
                   "dims": 384, "top_k": 10, "rows_per_gpu": 1_250_048, "parallelism": blah, "parallelism_short": "row-shard x8 rccl all_gather",
                   "pipeline_depth": 4, "timed_region": blah, "merge": "device", "exchange": "rccl all_gather", "rccl_ranks": 8, "shards": 8,
                   "last_result_checksum": "fedcba9876543210"},
        "roofline": roof,
        "cpu_baseline": {"value": 7.93, "unit": "queries/s", "cores": 16, "kind": "port", "sample": blah,
                         "sample_short": "95 queries over the first 1000000 rows in 12.0 s, x1000000/10000000 rows; 122 GB/s",
                         "variants": [{"threads": 1, "value": 0.53, "sample": blah}, {"threads": 16, "value": 7.93, "sample": blah}]},
        "secondary": sec,
    }


def test_bench_line_stays_inside_the_drivers_stdout_tail(tmp_path, capsys):
    """The contract line must survive a bounded stdout tail: ONE line, < 4 KB, with every contract key, `roofline` and
    `cpu_baseline` — whatever prose the full record carries (that goes to the detail file). Round 3's line was 22 KB."""
    import json
    bench = _load_bench()
    full = _synthetic_full_record(bench, n_secondary=12)
    assert len(json.dumps(full)) > 20_000                      # the round-3 shape
    line = bench.compact_line(full)
    text = json.dumps(line, separators=(",", ":"))
    assert len(text) < bench.LINE_BUDGET == 4096, len(text)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config", "roofline", "cpu_baseline", "secondary"):
        assert key in line, key
    assert line["config"]["workload"].startswith("10M x 384") and line["config"]["rccl_ranks"] == 8 and line["config"]["checksum"] == "fedcba9876543210"
    assert set(line["roofline"]) == {"bound", "achieved", "peak", "unit", "frac", "pipeline_frac", "kernel", "kernel_avg_ms",
                                     "kernel_launches_timed", "algorithmic_bytes_per_launch", "traffic", "traffic_from"}
    assert line["roofline"]["traffic_from"] in ("live-pmc", "replayed-pmc")
    assert line["roofline"]["kernel"] == "wax::scan_kernel" and abs(line["roofline"]["frac"] - 0.873265) < 1e-6
    assert line["cpu_baseline"]["cores"] == 16 and line["cpu_baseline"]["kind"] == "port" and line["cpu_baseline"]["value_1_thread"] == 0.53
    assert all(set(x) <= {"name", "value", "ms_per_step", "frac", "kernel_avg_ms", "n_gpus", "ck", "blocking_ms", "error"} for x in line["secondary"])
    assert line["secondary"][-1]["name"] == "broken" and len(line["secondary"][-1]["error"]) <= 80
    # emit(): detail file written, stdout carries exactly one line, and that line parses and is the compact one
    detail = tmp_path / "detail.json"
    bench.emit(full, str(detail))
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and len(out) < 4096 and json.loads(out)["value"] == 460.412
    assert json.load(open(detail))["roofline"]["note"] == "x" * 1200
    # an absurd record (60 secondaries) still yields a bounded line: the secondaries are dropped, never the headline
    bench.emit(_synthetic_full_record(bench, n_secondary=60), str(detail))
    out = capsys.readouterr().out
    j = json.loads(out)
    assert len(out) < 4096 and "secondary_dropped" in j and j["roofline"]["frac"] and j["cpu_baseline"]["cores"] == 16


def test_bench_plain_run_is_lean_by_default_and_dumps_float_arrays(tmp_path, monkeypatch):
    """`--full` (checks, roofline, CPU baseline, secondaries) is off unless asked for; `--dump-outputs DIR` writes the last step's
    answer as DIR/ids.npy (float64, exact for uint64 row keys below 2**53) and DIR/scores.npy (float32)."""
    import sys
    bench = _load_bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"])
    a = bench.parse_args()
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 3
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", str(tmp_path / "d")])
    a = bench.parse_args()
    assert a.full is True and a.dump_outputs == str(tmp_path / "d")
    ids = np.array([9_999_999, 123_457, 2**52 + 1], dtype=np.uint64)
    scores = np.array([0.5, 0.25, -0.125], dtype=np.float32)
    assert bench.dump_outputs(a.dump_outputs, ids, scores) == ["ids", "scores"]
    got_ids, got_scores = np.load(tmp_path / "d" / "ids.npy"), np.load(tmp_path / "d" / "scores.npy")
    assert got_ids.dtype == np.float64 and np.array_equal(got_ids.astype(np.uint64), ids)
    assert got_scores.dtype == np.float32 and np.array_equal(got_scores, scores)


def test_bench_line_carries_the_event_mode_and_the_bracketed_figure():
    """Round 5: `frac` is priced with kernel-bound HIP events (hipExtLaunchKernel start / stop pair on the dispatch); the line says
    which events it used and carries the bracketed mean (hipEventRecord around the launch) beside it; the plausibility rule that
    guards the switch refuses a pair the runtime did not bind."""
    import json
    bench = _load_bench()
    full = _synthetic_full_record(bench, n_secondary=11)
    full["roofline"] = dict(full["roofline"], calibration={"steps": 60, "events": "kernel-bound", "kernel_avg_ms_bracketed": 2.2112345678,
                                                           "kernel_avg_ms_kernel_bound": 2.1987654321})
    full["secondary"][0]["roofline"] = dict(full["secondary"][0]["roofline"], calibration={"events": "kernel-bound", "kernel_avg_ms_bracketed": 0.2959})
    r1 = {k: v for k, v in full["secondary"][1]["roofline"].items() if k != "calibration"}
    full["secondary"][1]["roofline"] = dict(r1, events="kernel-bound", kernel_avg_ms_bracketed=0.20412345)
    line = bench.compact_line(full)
    assert len(json.dumps(line, separators=(",", ":"))) < bench.LINE_BUDGET
    assert line["roofline"]["events"] == "kernel-bound" and line["roofline"]["kernel_avg_ms_bracketed"] == 2.21123
    assert line["secondary"][0]["bracketed_ms"] == 0.2959 and line["secondary"][1]["bracketed_ms"] == 0.2041
    assert "bracketed_ms" not in line["secondary"][2]
    ok = bench.kernel_bound_plausible
    assert ok(2.1744, 2.1874) and ok(0.284, 0.2959) and ok(0.0160, 0.0268) and ok(0.186, 0.194)
    assert not ok(0.0, 0.2959) and not ok(float("nan"), 0.2959) and not ok(0.31, 0.2959) and not ok(0.1, 0.2959) and not ok(1.9, 2.1874)
    # short kernels: a near-zero interval from a runtime that did not bind the pair is refused (relative floor), and so is one that
    # would put the launch above the peak rate (floor = algorithmic bytes / peak)
    assert not ok(0.0005, 0.0268) and not ok(0.006, 0.0268) and ok(0.0160, 0.0268, floor_ms=0.00192) and not ok(0.0160, 0.0268, floor_ms=0.02)
    # a bracket that carries half a millisecond the dispatch does not (the k > 192 queries): the bound interval stands while it is
    # physically possible (>= the bytes at the peak rate); without a floor the relative rule decides as before
    assert ok(2.1914, 2.7638, floor_ms=1.92) and not ok(2.1914, 2.7638) and not ok(1.8, 2.7638, floor_ms=1.92) and not ok(0.6, 2.7638, floor_ms=0.5)


def test_bench_secondary_watchdog_emits_the_headline_and_leaves(tmp_path):
    """A secondary that never returns (at N > 1: a collective one rank never joins) must not lose the headline: after the limit rank 0
    prints the ONE line with what has finished and an entry that says so, and the process exits with code 0; the other ranks only leave."""
    import json
    import subprocess
    import sys
    import time
    prog = (
        "import sys, time, types; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from test_host_cpu import _load_bench, _synthetic_full_record\n"
        "bench = _load_bench()\n"
        "rank = int(sys.argv[1])\n"
        "out = _synthetic_full_record(bench, n_secondary=2) if rank == 0 else None\n"
        "args = types.SimpleNamespace(detail_out=%r)\n"
        "bench.arm_secondary_watchdog(out, args, rank, limit_s=0.3)\n"
        "time.sleep(60)\n"
        "print('never')\n") % (os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__))), str(tmp_path / "d.json"))
    t0 = time.time()
    r0 = subprocess.run([sys.executable, "-c", prog, "0"], capture_output=True, text=True, timeout=50)
    assert r0.returncode == 0 and time.time() - t0 < 40, (r0.returncode, r0.stderr[-400:])
    lines = [l for l in r0.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and "never" not in r0.stdout
    j = json.loads(lines[0])
    assert j["value"] == 460.412 and j["secondary"][-1]["name"] == "watchdog" and "still running" in j["secondary"][-1]["error"]
    r1 = subprocess.run([sys.executable, "-c", prog, "1"], capture_output=True, text=True, timeout=50)
    assert r1.returncode == 0 and r1.stdout.strip() == ""
    # a watchdog that is cancelled does nothing, and emit_once prints once
    bench = _load_bench()
    w = bench.arm_secondary_watchdog(None, None, 1, limit_s=0.2)
    w.cancel()
    time.sleep(0.4)


def _bf16_rne(x):
    """f32 -> bf16 (round to nearest even) -> f32, as f32_to_bf16_rne in common.h does it."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32)


def test_measured_bf16_certificate_bound_is_a_bound():
    """The round-4 cosine certificate bound (batch_prep_kernel): |q~.v~ - x_q.x_v| <= ||q~ - x_q|| (1 + 2^-8) + max_rows ||v~ - x_v||
    (+ accumulation / normalisation slack), with x the f32-normalised vectors and ~ their bf16 roundings. Checked in f64 against
    the true error on random, clustered and adversarial inputs (rows built so that the rounding errors line up with the query —
    the case Cauchy-Schwarz is tight for), and well below the worst case 2^-7 (the kernel uses the smaller of the two). Also shown: a
    vector whose every element sits just below a rounding midpoint at the bottom of its binade moves its own self-similarity by more
    than the constant rounds 1-3 took for the worst case."""
    rng = np.random.default_rng(3)
    dims = 384
    worst = (2.0 ** -7) * (1 + 2.0 ** -9) + dims * 5.97e-8 + 1e-6   # bf16 keeps 8 significant bits: 2^-8 per operand, 2^-7 per product
    old_constant = (2.0 ** -8) * (1 + 2.0 ** -10)                  # what rounds 1-3 used as "worst case": half of it
    exceeded_old = 0
    ratios = []
    for kind in ("gaussian", "clustered", "aligned", "binade_edges"):
        n = 4000
        if kind == "gaussian":
            rows = rng.standard_normal((n, dims))
        elif kind == "clustered":
            rows = rng.standard_normal((1, dims)) + 0.05 * rng.standard_normal((n, dims))
        elif kind == "binade_edges":                      # magnitudes just above powers of two: the largest relative bf16 error
            rows = np.sign(rng.standard_normal((n, dims))) * (2.0 ** rng.integers(-6, 0, (n, dims))) * (1 + 2.0 ** -9 * rng.uniform(0.9, 1.0, (n, dims)))
        else:
            rows = rng.standard_normal((n, dims))
        rows = rows.astype(np.float32)
        xv = (rows / np.sqrt(np.sum(rows.astype(np.float32) ** 2, axis=1, dtype=np.float32))[:, None]).astype(np.float32)   # f32 normalisation, like mirror_kernel
        vt = _bf16_rne(xv)
        err_v = np.sqrt(np.sum((xv.astype(np.float64) - vt.astype(np.float64)) ** 2, axis=1))
        for _ in range(40):
            q = rng.standard_normal(dims).astype(np.float32)
            if kind == "aligned":                          # the query points along a row's rounding-error vector
                i = rng.integers(0, n)
                q = (xv[i].astype(np.float64) - vt[i].astype(np.float64) + 1e-9 * rng.standard_normal(dims)).astype(np.float32)
            xq = (q / np.sqrt(np.sum(q * q, dtype=np.float32))).astype(np.float32)
            qt = _bf16_rne(xq)
            err_q = np.sqrt(np.sum((xq.astype(np.float64) - qt.astype(np.float64)) ** 2))
            true = np.abs(vt.astype(np.float64) @ qt.astype(np.float64) - xv.astype(np.float64) @ xq.astype(np.float64))
            bound = err_q * (1 + 1 / 256) + err_v.max() * 1.001 + 3 * dims * 5.97e-8 + 3e-6
            assert true.max() <= min(bound, worst), (kind, true.max(), bound, worst)   # the kernel takes the smaller of the two
            assert bound < worst, (kind, bound, worst)
            exceeded_old += true.max() > old_constant
            ratios.append(bound / worst)
    assert np.mean(ratios) < 0.6                           # ~0.46 of the worst case on embedding-like data
    # the adversarial construction really does exceed the old constant: every element just below a rounding midpoint at the bottom
    # of its binade (so that it loses 2^-8 of itself), magnitudes chosen so that the vector has unit norm without rescaling
    x = helpers.bf16_adversarial_unit_vector(dims)
    xt = _bf16_rne(x)
    err = float(np.abs(xt.astype(np.float64) @ xt.astype(np.float64) - x.astype(np.float64) @ x.astype(np.float64)))
    en = float(np.sqrt(np.sum((x.astype(np.float64) - xt.astype(np.float64)) ** 2)))
    assert old_constant < err <= en * (1 + 1 / 256) + en * 1.001 + 3 * dims * 5.97e-8 + 3e-6 and err <= worst
    print(f"\n[bf16 bound] self-similarity error of an adversarial vector {err:.5f} (old constant {old_constant:.5f}, worst case {worst:.5f}, measured bound {2 * en:.5f})")


def test_bench_reads_fetch_size_per_launch_from_a_counter_pass(tmp_path):
    """bench.live_traffic's reader: a rocprofv3 `--pmc FETCH_SIZE --output-format csv` directory -> FETCH_SIZE of the counted launches,
    in dispatch order, the two warm-ups dropped. Single-query pass: the scan kernel (either form), other kernels and counters ignored.
    Batched pass: of the `batch_gemm_*` instantiations, the one that streams the mirror (largest mean), not the sampling launch."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("wax_bench", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    d = tmp_path / "node" / "123"
    d.mkdir(parents=True)
    head = "Correlation_Id,Dispatch_Id,Agent_Id,Kernel_Name,Counter_Name,Counter_Value\n"
    rows = []
    for i in range(8):                                    # dispatches written out of order on purpose
        rows.append(f'{i},{20 - i},1,"void wax::scan_kernel<96, 32, 0, 4, true, 128, false>(wax::ScanArgs)",FETCH_SIZE,{7500000 + (20 - i)}\n')
        rows.append(f'{i},{20 - i},1,"void wax::scan_kernel<96, 32, 0, 4, true, 128, false>(wax::ScanArgs)",SQ_WAVES,5\n')
        rows.append(f'{i},{40 + i},1,"void wax::merge_keys_kernel<128>(long const*)",FETCH_SIZE,3\n')
    (d / "t_counter_collection.csv").write_text(head + "".join(rows))
    got = bench.fetch_size_per_launch(str(tmp_path), False)
    assert got == [7500000.0 + x for x in range(15, 21)]  # dispatch ids 13, 14 were the warm-ups
    assert sum(got) / len(got) * 2048 == (7500000 + 17.5) * 2048
    rows = []
    for i in range(5):
        rows.append(f'{i},{2 * i},1,"void wax::batch_gemm_rq_kernel<384, 64, 2, 3, true, false, false>(wax::GemmArgs, unsigned int)",FETCH_SIZE,{9000 + i}\n')
        rows.append(f'{i},{2 * i + 1},1,"void wax::batch_gemm_rq_kernel<384, 64, 2, 3, false, true, true>(wax::GemmArgs, unsigned int)",FETCH_SIZE,{375000 + i}\n')
    (d / "t_counter_collection.csv").write_text(head + "".join(rows))
    assert bench.fetch_size_per_launch(str(tmp_path), True) == [375002.0, 375003.0, 375004.0]
    assert bench.fetch_size_per_launch(str(tmp_path), False) == []     # no scan kernel in a batched pass


def test_bench_counter_passes_are_bounded():
    """bench.py's live counter passes are an optional leg of a run that must finish within minutes: a pass that hits its limit
    disables the rest, and all passes together have a budget; after either, live_traffic returns at once with the reason (the
    caller falls back to the replayed figure)."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("wax_bench", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    assert bench.live_allowed() is None
    for _ in range(5):
        bench.live_account(12.0)
    assert bench.live_allowed() is None and bench.LIVE_STATE["passes"] == 5
    bench.live_account(bench.LIVE_TOTAL_BUDGET_S)                       # budget spent
    assert "budget" in bench.live_allowed()
    bench.LIVE_STATE.update(disabled=None, spent_s=0.0, passes=0)
    bench.live_account(bench.LIVE_CHILD_LIMIT_S, timed_out=True)        # one pass hung: no more passes in this run
    why = bench.live_allowed()
    assert why and "disabled" in why
    import shutil
    if shutil.which("rocprofv3") or os.path.exists("/opt/rocm/bin/rocprofv3"):
        got, note = bench.live_traffic(1000, 384, 10)                   # returns at once, nothing is launched
        assert got is None and "disabled" in note



def test_every_tuning_key_is_documented_in_the_header():
    """include/wax_hip.h is the only interface: every key wax_hip_set_tuning / wax_hip_get_tuning accept (the table in tuning.inc, and the
    sharded handle's own keys in sharded.inc) is named in its comment block — a key a maintainer cannot find does not exist."""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "wax_amd", "csrc", "tuning.inc")) as f:
        keys = set(re.findall(r'^ *\{"([a-z0-9_]+)",', f.read(), re.M))                  # the rows of the table: every key of an engine
    with open(os.path.join(root, "wax_amd", "csrc", "sharded.inc")) as f:
        keys |= set(re.findall(r'k == "([a-z0-9_]+)"', f.read()))                        # the handle's own, still branches
    keys = sorted(keys)
    assert len(keys) >= 60
    with open(os.path.join(root, "include", "wax_hip.h")) as f:
        header = f.read()
    missing = [k for k in keys if f'"{k}"' not in header]
    assert not missing, missing
