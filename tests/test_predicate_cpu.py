"""Per-row attributes and the predicate search (wax_hip_set_attributes / wax_hip_get_attributes / wax_hip_search_predicate), the
parts that need no GPU: the symbols are exported and bound, the header, the ctypes table and the Python wrapper agree on them."""
import ctypes
import inspect
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("wax_hip_set_attributes", "wax_hip_get_attributes", "wax_hip_search_predicate")


def header_text():
    return open(os.path.join(ROOT, "include", "wax_hip.h")).read()


def test_library_exports_the_three_symbols(hip_lib):
    for name, nargs in zip(NEW, (6, 6, 14)):
        fn = getattr(hip_lib, name)
        assert fn.restype is ctypes.c_int
        assert len(fn.argtypes) == nargs, name


def test_header_and_signatures_agree(hip_lib):
    from wax_amd import _abi
    declared = _abi.declared_symbols()
    code = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    for name in NEW:
        assert name in declared and name in _abi.SIGNATURES
        m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m, f"the header does not declare {name}"
        assert len(m.group(1).split(",")) == len(_abi.SIGNATURES[name][1]), name
    assert re.search(r"#define\s+WAX_HIP_ABI_VERSION\s+2\b", header_text()), "adding symbols keeps the ABI version"
    assert hip_lib.wax_hip_abi_version() == 2


def test_predicate_struct_and_flag_bits_match_the_header():
    from wax_amd import _abi
    h = header_text()
    m = re.search(r"typedef struct wax_hip_row_predicate \{(.*?)\} wax_hip_row_predicate;", h, flags=re.S)
    assert m, "the header does not define wax_hip_row_predicate"
    fields = re.findall(r"(\w+)\s+(\w+);", m.group(1))
    assert fields == [("int32_t", "has_after"), ("int64_t", "after"), ("int32_t", "has_before"), ("int64_t", "before"),
                      ("uint32_t", "deny_flags")]
    assert [f[0] for f in _abi.RowPredicate._fields_] == [name for _, name in fields]
    assert ctypes.sizeof(_abi.RowPredicate) == 40       # natural alignment of {i32, i64, i32, i64, u32}
    for macro, value in (("WAX_HIP_FLAG_DELETED", _abi.FLAG_DELETED), ("WAX_HIP_FLAG_SUPERSEDED", _abi.FLAG_SUPERSEDED),
                         ("WAX_HIP_FLAG_SURROGATE", _abi.FLAG_SURROGATE), ("WAX_HIP_FLAG_USER_SHIFT", _abi.FLAG_USER_SHIFT)):
        d = re.search(r"#define\s+" + macro + r"\s+(0x[0-9a-fA-F]+|\d+)u?\b", h)
        assert d and int(d.group(1), 0) == value, macro
    assert (_abi.FLAG_DELETED, _abi.FLAG_SUPERSEDED, _abi.FLAG_SURROGATE, _abi.FLAG_USER_SHIFT) == (1, 2, 4, 8)


def test_python_signatures_accept_the_new_arguments():
    from wax_amd import HIPVectorEngine
    sf = inspect.signature(HIPVectorEngine.searchFiltered).parameters
    assert list(sf)[:5] == ["self", "vector", "topK", "frameIds", "minScore"], "the existing arguments keep their places"
    assert sf["timeRange"].default is None and sf["denyFlags"].default == 0
    sa = inspect.signature(HIPVectorEngine.setAttributes).parameters
    assert list(sa) == ["self", "frameIds", "timestamps", "flags"] and sa["timestamps"].default is None and sa["flags"].default is None
    assert list(inspect.signature(HIPVectorEngine.getAttributes).parameters) == ["self", "frameIds"]


def test_null_arguments_are_refused(hip_lib):
    ids = np.array([1, 2, 3], dtype=np.uint64)
    u64 = ctypes.POINTER(ctypes.c_uint64)
    applied = ctypes.c_uint64(77)
    assert hip_lib.wax_hip_set_attributes(None, ids.ctypes.data_as(u64), None, None, 3, ctypes.byref(applied)) == -7
    assert applied.value == 0                              # *out_applied cleared
    assert b"engine is null" in hip_lib.wax_hip_last_error()
    assert hip_lib.wax_hip_get_attributes(None, ids.ctypes.data_as(u64), 3, None, None, None) == -7
    got = ctypes.c_uint32(5)
    q = np.zeros(8, dtype=np.float32)
    rc = hip_lib.wax_hip_search_predicate(None, q.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 8, 10, 0, None, 0, 0, 0.0, None,
                                          None, None, 0, ctypes.byref(got))
    assert rc == -7 and got.value == 0


def test_wrapper_routes_by_the_new_arguments():
    """searchFiltered without timeRange / denyFlags calls the old entry with the old arguments; with either it calls the predicate
    entry with the same arguments plus the predicate struct."""
    import wax_amd
    from wax_amd import _abi

    calls = []

    class FakeLib:
        def wax_hip_count(self, h):
            return 100

        def wax_hip_search_filtered(self, *a):
            calls.append(("filtered", a))
            return 0

        def wax_hip_search_predicate(self, *a):
            calls.append(("predicate", a))
            return 0

    eng = object.__new__(wax_amd.HIPVectorEngine)
    eng._lib, eng._h, eng.dimensions = FakeLib(), ctypes.c_void_p(1), 4
    try:
        q = np.ones(4, dtype=np.float32)
        eng.searchFiltered(q, 5, frameIds=[1, 2], minScore=0.5)
        eng.searchFiltered(q, 5, frameIds=[1, 2], minScore=0.5, timeRange=(None, 7), denyFlags=_abi.FLAG_DELETED | (1 << 9))
        eng.searchFiltered(q, 5, timeRange=(-3, None))
        assert [c[0] for c in calls] == ["filtered", "predicate", "predicate"]
        old, new = calls[0][1], calls[1][1]
        assert len(old) == 13 and len(new) == 14
        assert old[2:5] == new[2:5] == (4, 5, 1) and old[6:9] == new[6:9] == (2, 1, 0.5)
        p = new[9]._obj
        assert (p.has_after, p.has_before, p.before, p.deny_flags) == (0, 1, 7, 0x201)
        p = calls[2][1][9]._obj
        assert (p.has_after, p.after, p.has_before, p.deny_flags) == (1, -3, 0, 0)
    finally:
        eng._h = ctypes.c_void_p()      # nothing to destroy
