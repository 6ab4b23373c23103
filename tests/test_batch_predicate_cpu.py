"""Batched predicate search, host side: wax_hip_search_batch_predicate is declared, bound and exported, refuses what the batched
filtered call refuses, and searchBatchFiltered takes the per-query timeRange / denyFlags of searchManyFiltered.

What needs a live engine (nq == 0 returning OK with null arrays, allow_begin without allow_len, a range that leaves the id array)
comes behind the null-engine test in the call's fixed order, so without a device only that order can be shown here;
test_batch_predicate_gpu.py::test_refusals checks them, with their messages, where an engine exists."""
import ctypes
import inspect

import numpy as np
import pytest

from wax_amd import _abi

U64 = ctypes.POINTER(ctypes.c_uint64)
U32 = ctypes.POINTER(ctypes.c_uint32)
F32 = ctypes.POINTER(ctypes.c_float)


def test_symbol_is_declared_bound_and_exported(hip_lib):
    name = "wax_hip_search_batch_predicate"
    assert name in _abi.declared_symbols()
    assert name in _abi.SIGNATURES
    restype, argtypes = _abi.SIGNATURES[name]
    assert restype is ctypes.c_int and len(argtypes) == 15
    assert argtypes[10] == ctypes.POINTER(_abi.RowPredicate)            # preds sits between min_scores and the outputs
    assert argtypes[:10] == _abi.SIGNATURES["wax_hip_search_batch_filtered"][1][:10]
    assert argtypes[11:] == _abi.SIGNATURES["wax_hip_search_batch_filtered"][1][10:]
    assert hasattr(hip_lib, name)


def test_abi_version_is_still_2(hip_lib):
    assert hip_lib.wax_hip_abi_version() == 2
    with open(_abi.HEADER_PATH) as f:
        assert "#define WAX_HIP_ABI_VERSION 2" in f.read()


def test_null_engine_is_refused_first_and_outputs_stay(hip_lib):
    q = np.zeros((2, 8), np.float32)
    cnt = np.full(2, 77, np.uint32)
    ids = np.full((2, 4), 55, np.uint64)
    sc = np.full((2, 4), 5.5, np.float32)
    flat = np.arange(4, dtype=np.uint64)
    begin = np.zeros(2, np.uint64)
    length = np.full(2, 9, np.uint64)          # leaves the id array: the null engine is still what is reported
    preds = (_abi.RowPredicate * 2)()
    for args in ((None, 0, None, None), (flat.ctypes.data_as(U64), 4, begin.ctypes.data_as(U64), None),
                 (flat.ctypes.data_as(U64), 4, begin.ctypes.data_as(U64), length.ctypes.data_as(U64))):
        rc = hip_lib.wax_hip_search_batch_predicate(None, q.ctypes.data_as(F32), 2, 8, 10, *args, None, preds,
                                                    ids.ctypes.data_as(U64), sc.ctypes.data_as(F32), 4, cnt.ctypes.data_as(U32))
        assert rc == _abi.ERR_INVALID_ARGUMENT
        assert _abi.last_error() == "engine is null"
        assert (cnt == 77).all() and (ids == 55).all() and (sc == 5.5).all()
    # the same words as the call it extends
    rc = hip_lib.wax_hip_search_batch_filtered(None, q.ctypes.data_as(F32), 2, 8, 10, None, 0, None, None, None,
                                               ids.ctypes.data_as(U64), sc.ctypes.data_as(F32), 4, cnt.ctypes.data_as(U32))
    assert rc == _abi.ERR_INVALID_ARGUMENT and _abi.last_error() == "engine is null"


def test_python_takes_the_new_keywords():
    from wax_amd import HIPVectorEngine
    params = inspect.signature(HIPVectorEngine.searchBatchFiltered).parameters
    assert list(params)[1:] == ["vectors", "topK", "frameIds", "minScore", "timeRange", "denyFlags"]
    assert params["timeRange"].default is None and params["denyFlags"].default == 0


def test_per_query_filters_follow_search_many_filtered():
    from wax_amd import EncodingError
    from wax_amd.engine import _per_pair, _row_predicates
    who = dict(who="searchBatchFiltered", per="query")
    assert _per_pair((5, None), 3, "timeRange", tuple_is_value=True, **who) == [(5, None)] * 3         # one tuple is one value
    assert _per_pair([(5, None), None, (None, 9)], 3, "timeRange", tuple_is_value=True, **who) == [(5, None), None, (None, 9)]
    assert _per_pair(7, 2, "denyFlags", **who) == [7, 7]
    with pytest.raises(EncodingError) as ei:
        _per_pair([1, 2], 3, "denyFlags", **who)
    assert "searchBatchFiltered" in str(ei.value) and "per query" in str(ei.value)
    with pytest.raises(EncodingError):
        _per_pair([(1, 2)] * 4, 3, "timeRange", tuple_is_value=True, **who)
    preds = _row_predicates([(5, None), None, (None, -9)], [0, None, 0x104])
    got = [(p.has_after, p.after, p.has_before, p.before, p.deny_flags) for p in preds]
    assert got == [(1, 5, 0, 0, 0), (0, 0, 0, 0, 0), (0, 0, 1, -9, 0x104)]


class _NoEngine:
    """searchBatchFiltered up to the C call, without a device: the argument handling is pure Python."""
    count = 100
    _h = None

    class _Lib:
        def __getattr__(self, name):
            raise AssertionError(f"{name} must not be reached")
    _lib = _Lib()


def test_wrong_length_lists_raise_before_any_call():
    from wax_amd import EncodingError, HIPVectorEngine
    q = np.zeros((3, 8), np.float32)
    for kw in (dict(timeRange=[(1, 2), None]), dict(denyFlags=[1, 2, 3, 4]), dict(timeRange=[None] * 3, denyFlags=np.array([1, 2]))):
        with pytest.raises(EncodingError) as ei:
            HIPVectorEngine.searchBatchFiltered(_NoEngine(), q, 10, **kw)
        assert "one entry per query" in str(ei.value)


def test_new_tuning_keys_are_documented_and_summed_over_shards():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "wax_hip.h")).read()
    tuning = open(os.path.join(root, "wax_amd", "csrc", "tuning.inc")).read()
    import re
    rows = dict(re.findall(r'^ *\{"([a-z_0-9]+)",(.*)$', tuning, re.M))   # the tuning table: {"name", how to set, how to get, what a sharded handle answers}
    for key in ("predicate_batch_rows", "predicate_batch_queries", "predicate_batch_classes"):
        assert f'"{key}"' in header and key in rows
    assert "not_set()" not in rows["predicate_batch_rows"]
    for key in ("predicate_batch_queries", "predicate_batch_classes"):   # counters: not settable, summed over the shards
        assert "not_set()" in rows[key] and "not_get()" not in rows[key] and re.search(r"SUM_SHARDS\},", rows[key])
