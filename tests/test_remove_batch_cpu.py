"""removeBatch (wax_hip_remove_batch), the parts that need no GPU: the symbol is exported and bound, the header, the ctypes table and
the Python / C++ / Swift wrappers agree on it, and the header documents the new tuning keys."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_text():
    return open(os.path.join(ROOT, "include", "wax_hip.h")).read()


def test_library_exports_remove_batch(hip_lib):
    fn = getattr(hip_lib, "wax_hip_remove_batch")
    assert fn.restype is ctypes.c_int
    assert len(fn.argtypes) == 4


def test_header_and_signatures_agree():
    from wax_amd import _abi
    assert "wax_hip_remove_batch" in _abi.declared_symbols()
    restype, argtypes = _abi.SIGNATURES["wax_hip_remove_batch"]
    assert restype is ctypes.c_int
    u64p = ctypes.POINTER(ctypes.c_uint64)
    assert argtypes == [ctypes.c_void_p, u64p, ctypes.c_uint64, u64p]
    m = re.search(r"int\s+wax_hip_remove_batch\s*\(([^)]*)\)\s*;", header_text())
    assert m, "the header does not declare wax_hip_remove_batch"
    args = [a.strip() for a in m.group(1).split(",")]
    assert args == ["wax_hip_engine* e", "const uint64_t* frame_ids", "uint64_t n", "uint64_t* out_removed"]
    assert re.search(r"#define\s+WAX_HIP_ABI_VERSION\s+2\b", header_text()), "adding a symbol keeps the ABI version"


def test_null_engine_and_null_ids_are_refused(hip_lib):
    removed = ctypes.c_uint64(77)
    ids = np.array([1, 2, 3], dtype=np.uint64)
    rc = hip_lib.wax_hip_remove_batch(None, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), 3, ctypes.byref(removed))
    assert rc == -7 and removed.value == 0      # WAX_HIP_ERR_INVALID_ARGUMENT, *out_removed cleared
    assert b"engine is null" in hip_lib.wax_hip_last_error()


def test_python_wrapper_packs_uint64_ids():
    """HIPVectorEngine.removeBatch hands the library a contiguous uint64 array, its length and an out-parameter, whatever sequence
    type the caller used, and reports the library's count; an empty list never reaches the library."""
    import wax_amd
    from wax_amd import engine as engine_mod

    calls = []

    class FakeLib:
        def wax_hip_remove_batch(self, h, ids_p, n, out):
            arr = np.ctypeslib.as_array(ids_p, shape=(n,)).copy()
            calls.append((arr, n))
            ctypes.cast(out, ctypes.POINTER(ctypes.c_uint64))[0] = n - 1
            return 0

    eng = object.__new__(wax_amd.HIPVectorEngine)
    eng._lib, eng._h, eng._dirty = FakeLib(), ctypes.c_void_p(1), False
    try:
        assert hasattr(engine_mod.HIPVectorEngine, "removeBatch")
        assert eng.removeBatch([]) == 0 and not calls and not eng._dirty
        big = 2 ** 63 + 5                                   # does not fit a signed 64-bit integer
        assert eng.removeBatch([3, big, 3]) == 2
        arr, n = calls[-1]
        assert n == 3 and arr.dtype == np.uint64 and arr.tolist() == [3, big, 3]
        assert eng._dirty
        eng._dirty = False
        assert eng.removeBatch(np.array([[9, 8], [7, 6]], dtype=np.int32)[:, 0]) == 1     # a strided int32 view
        arr, n = calls[-1]
        assert n == 2 and arr.dtype == np.uint64 and arr.tolist() == [9, 7]
    finally:
        eng._h = ctypes.c_void_p()                          # nothing to destroy


def test_header_documents_the_new_tuning_keys():
    text = header_text()
    block = text[text.index("Tunables (all optional)"):text.index("int wax_hip_set_tuning")]
    for key in ("compact_window_rows", "remove_batches", "remove_batch_rows", "remove_batch_bytes_written"):
        assert f'"{key}"' in block, f"the tunables block does not document {key}"


def test_cpp_and_swift_wrappers_call_it():
    hpp = open(os.path.join(ROOT, "include", "wax_hip.hpp")).read()
    assert "removeBatch(" in hpp and "wax_hip_remove_batch(h_, frameIds.data(), frameIds.size(), &removed)" in hpp
    swift = open(os.path.join(ROOT, "swift", "HIPVectorEngine.swift")).read()
    assert "public func removeBatch(frameIds: [UInt64]) async throws -> Int" in swift
    assert "wax_hip_remove_batch(h.raw, ids.baseAddress, UInt64(ids.count), &n)" in swift


def test_source_list_builds_the_compaction_unit():
    from wax_amd import build
    assert "compact.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "compact.hip"))
