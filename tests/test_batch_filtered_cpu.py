"""Batched filtered search, host side: the entry point is exported and declared, the Python packing of per-query allow-lists, and
the loud errors without a device."""
import ctypes

import numpy as np
import pytest

from wax_amd import _abi
from wax_amd.engine import pack_allow_lists


def test_symbol_is_exported_and_declared(hip_lib):
    assert "wax_hip_search_batch_filtered" in _abi.SIGNATURES
    assert "wax_hip_search_batch_filtered" in _abi.declared_symbols()
    assert hasattr(hip_lib, "wax_hip_search_batch_filtered")
    with open(_abi.HEADER_PATH) as f:
        header = f.read()
    assert "#define WAX_HIP_NO_ALLOW_LIST UINT64_MAX" in header
    assert _abi.NO_ALLOW_LIST == 2 ** 64 - 1


def test_packing_shares_repeated_lists():
    shared = [5, 6, 7]
    other = np.array([9, 10], dtype=np.uint64)
    flat, begin, length = pack_allow_lists([shared, None, other, shared, [], None], 6)
    assert flat.dtype == np.uint64 and flat.tolist() == [5, 6, 7, 9, 10]
    assert begin[0] == begin[3] == 0 and length[0] == length[3] == 3          # one range for the repeated object
    assert begin[2] == 3 and length[2] == 2
    assert length[4] == 0                                                     # empty list: nothing allowed
    assert length[1] == length[5] == _abi.NO_ALLOW_LIST                      # None: no list
    flat, begin, length = pack_allow_lists(None, 3)
    assert flat.size == 0 and begin is None and length is None
    with pytest.raises(Exception):
        pack_allow_lists([[1]], 2)


def test_without_a_device_the_call_is_refused(hip_lib):
    import wax_amd
    u64 = ctypes.POINTER(ctypes.c_uint64)
    u32 = ctypes.POINTER(ctypes.c_uint32)
    f32 = ctypes.POINTER(ctypes.c_float)
    q = np.zeros((2, 8), np.float32)
    cnt = np.zeros(2, np.uint32)
    rc = hip_lib.wax_hip_search_batch_filtered(None, q.ctypes.data_as(f32), 2, 8, 10, None, 0, None, None, None,
                                               None, None, 0, cnt.ctypes.data_as(u32))
    assert rc == _abi.ERR_INVALID_ARGUMENT
    if hip_lib.wax_hip_device_count() == 0:
        with pytest.raises(wax_amd.InvalidToc):
            wax_amd.HIPVectorEngine(dimensions=8)
    del u64
