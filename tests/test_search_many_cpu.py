"""wax_hip_search_many / searchMany, host side: the entry point is declared, bound and exported, and the two answers it gives
before it touches a device."""
import ctypes
import re

import numpy as np

from wax_amd import _abi


def test_symbol_is_declared_bound_and_exported(hip_lib):
    assert "wax_hip_search_many" in _abi.declared_symbols()
    assert len(_abi.SIGNATURES["wax_hip_search_many"][1]) == 9
    assert hasattr(hip_lib, "wax_hip_search_many")
    header = re.sub(r"/\*.*?\*/", "", open(_abi.HEADER_PATH).read(), flags=re.S)
    m = re.search(r"\bwax_hip_search_many\s*\(([^)]*)\)", header)
    assert m and len(m.group(1).split(",")) == 9


def test_no_pairs_is_ok_with_null_arrays(hip_lib):
    assert hip_lib.wax_hip_search_many(None, None, 0, 384, 10, None, None, 0, None) == _abi.OK


def test_a_null_engine_is_refused_by_index(hip_lib):
    f32 = ctypes.POINTER(ctypes.c_float)
    u32 = ctypes.POINTER(ctypes.c_uint32)
    u64 = ctypes.POINTER(ctypes.c_uint64)
    handles = (ctypes.c_void_p * 2)(None, None)
    q = np.zeros((2, 8), np.float32)
    ids = np.full((2, 4), 7, np.uint64)
    scores = np.full((2, 4), 7, np.float32)
    counts = np.full(2, 7, np.uint32)
    rc = hip_lib.wax_hip_search_many(handles, q.ctypes.data_as(f32), 2, 8, 4, ids.ctypes.data_as(u64), scores.ctypes.data_as(f32), 4,
                                     counts.ctypes.data_as(u32))
    assert rc == _abi.ERR_INVALID_ARGUMENT
    assert "pair 0" in _abi.last_error() and "null" in _abi.last_error()
    assert (ids == 7).all() and (scores == 7).all() and (counts == 7).all()     # refused before anything was written


def test_python_entry_is_exported():
    import wax_amd
    assert callable(wax_amd.searchMany) and "searchMany" in wax_amd.__all__
