"""wax_hip_search_many_predicate / searchManyFiltered, host side: the entry point is declared, bound and exported under the same
ABI version, and the two answers it gives before it touches a device."""
import ctypes
import re

import numpy as np

from wax_amd import _abi

NAME = "wax_hip_search_many_predicate"


def test_symbol_is_declared_bound_and_exported(hip_lib):
    assert NAME in _abi.declared_symbols()
    assert len(_abi.SIGNATURES[NAME][1]) == 11
    assert hasattr(hip_lib, NAME)
    text = open(_abi.HEADER_PATH).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\b" + NAME + r"\s*\(([^)]*)\)", header)
    assert m and len(m.group(1).split(",")) == 11
    assert re.search(r"#define\s+WAX_HIP_ABI_VERSION\s+2\b", text)      # a new function, not a new ABI
    assert hip_lib.wax_hip_abi_version() == 2


def test_no_pairs_is_ok_with_null_arrays(hip_lib):
    assert getattr(hip_lib, NAME)(None, None, 0, 384, 10, None, None, None, None, 0, None) == _abi.OK


def test_a_null_engine_is_refused_by_index(hip_lib):
    f32 = ctypes.POINTER(ctypes.c_float)
    u32 = ctypes.POINTER(ctypes.c_uint32)
    u64 = ctypes.POINTER(ctypes.c_uint64)
    handles = (ctypes.c_void_p * 2)(None, None)
    q = np.zeros((2, 8), np.float32)
    preds = (_abi.RowPredicate * 2)(_abi.RowPredicate(0, 0, 0, 0, 7), _abi.RowPredicate(1, 5, 0, 0, 0))
    cuts = np.array([0.5, np.nan], np.float32)
    ids = np.full((2, 4), 7, np.uint64)
    scores = np.full((2, 4), 7, np.float32)
    counts = np.full(2, 7, np.uint32)
    rc = getattr(hip_lib, NAME)(handles, q.ctypes.data_as(f32), 2, 8, 4, preds, cuts.ctypes.data_as(f32), ids.ctypes.data_as(u64),
                                scores.ctypes.data_as(f32), 4, counts.ctypes.data_as(u32))
    assert rc == _abi.ERR_INVALID_ARGUMENT
    assert "pair 0" in _abi.last_error() and "null" in _abi.last_error()
    assert (ids == 7).all() and (scores == 7).all() and (counts == 7).all()     # refused before anything was written


def test_python_entry_is_exported():
    import wax_amd
    assert callable(wax_amd.searchManyFiltered) and "searchManyFiltered" in wax_amd.__all__
