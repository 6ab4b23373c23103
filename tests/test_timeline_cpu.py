"""The timeline lane (wax_hip_timeline / wax_hip_timeline_device / wax_hip_timeline_probe), the parts that need no GPU: the symbols
are declared, bound and exported, refusals leave the outputs alone, and the shared case table (tests/timeline_ref.py) is not vacuous —
its tie cases tell frame-id ties from row ties, its boundary cases sit on the bounds, its counts are what the cases claim."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import timeline_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"wax_hip_timeline": 8, "wax_hip_timeline_device": 7, "wax_hip_timeline_probe": 11}
INVALID_ARGUMENT = -7


def header_text():
    return open(os.path.join(ROOT, "include", "wax_hip.h")).read()


def test_symbols_are_declared_bound_and_exported(hip_lib):
    from wax_amd import _abi
    declared = _abi.declared_symbols()
    code = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    for name, nargs in NEW.items():
        assert name in declared and name in _abi.SIGNATURES
        fn = getattr(hip_lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs, name
        m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m, f"the header does not declare {name}"
        assert len(m.group(1).split(",")) == nargs, name
    assert re.search(r"#define\s+WAX_HIP_ABI_VERSION\s+2\b", header_text()), "adding symbols keeps the ABI version"
    assert hip_lib.wax_hip_abi_version() == 2
    d = re.search(r"#define\s+WAX_HIP_TIMELINE_MAX_LIMIT\s+(\d+)", header_text())
    r = re.search(r"#define\s+WAX_HIP_RRF_MAX_ENTRIES\s+(\d+)", header_text())
    assert d and r and int(d.group(1)) == int(r.group(1)) == ref.MAX_LIMIT, "a longer lane could not be fused"


def test_python_surface():
    import wax_amd
    from wax_amd import HIPVectorEngine
    assert wax_amd.TIMELINE_MAX_LIMIT == ref.MAX_LIMIT
    for name in ("timelineProbe", "TIMELINE_MAX_LIMIT"):
        assert name in wax_amd.__all__ and hasattr(wax_amd, name)
    p = inspect.signature(HIPVectorEngine.timeline).parameters
    assert list(p) == ["self", "limit", "newestFirst", "timeRange", "denyFlags"]
    assert p["newestFirst"].default is True and p["timeRange"].default is None and p["denyFlags"].default == 0
    d = inspect.signature(HIPVectorEngine.timelineDevice).parameters
    assert {"limit", "out_ids", "out_count", "newestFirst", "timeRange", "denyFlags", "stream"} <= set(d)


def test_null_engine_and_null_outputs_are_refused_and_outputs_left_alone(hip_lib):
    u64, i64, u32 = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_uint32)
    ids = np.full(4, 11, dtype=np.uint64)
    ts = np.full(4, 22, dtype=np.int64)
    got = ctypes.c_uint32(55)
    rc = hip_lib.wax_hip_timeline(None, 4, 1, None, ids.ctypes.data_as(u64), ts.ctypes.data_as(i64), 4, ctypes.byref(got))
    assert rc == INVALID_ARGUMENT and b"engine is null" in hip_lib.wax_hip_last_error()
    assert got.value == 55 and ids.tolist() == [11] * 4 and ts.tolist() == [22] * 4
    rc = hip_lib.wax_hip_timeline_device(None, 4, 1, None, None, None, None)
    assert rc == INVALID_ARGUMENT and b"engine is null" in hip_lib.wax_hip_last_error()
    # the probe: no ids out, no count out, rows without frame ids
    fid = np.arange(4, dtype=np.uint64)
    for out_ids, out_count, frame_ids in ((None, ctypes.byref(got), fid.ctypes.data_as(u64)),
                                          (ids.ctypes.data_as(u64), None, fid.ctypes.data_as(u64)),
                                          (ids.ctypes.data_as(u64), ctypes.byref(got), None)):
        rc = hip_lib.wax_hip_timeline_probe(None, None, frame_ids, 4, 4, 1, None, 1, out_ids, ts.ctypes.data_as(i64), out_count)
        assert rc == INVALID_ARGUMENT and b"null argument" in hip_lib.wax_hip_last_error()
        assert got.value == 55 and ids.tolist() == [11] * 4 and ts.tolist() == [22] * 4


def test_limit_above_the_maximum_is_refused_before_any_device_is_touched(hip_lib):
    import wax_amd
    u64, i64 = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int64)
    fid = np.arange(4, dtype=np.uint64)
    ids = np.full(ref.MAX_LIMIT + 1, 11, dtype=np.uint64)
    got = ctypes.c_uint32(55)
    rc = hip_lib.wax_hip_timeline_probe(None, None, fid.ctypes.data_as(u64), 4, ref.MAX_LIMIT + 1, 1, None, 0, ids.ctypes.data_as(u64), None,
                                        ctypes.byref(got))
    assert rc == INVALID_ARGUMENT and b"4096" in hip_lib.wax_hip_last_error()
    assert got.value == 55 and bool(np.all(ids == 11))
    with pytest.raises(wax_amd.WaxError):
        wax_amd.timelineProbe(None, None, fid, ref.MAX_LIMIT + 1)
    # limit <= 0 is an answer (TimelineQuery.swift:51), and needs no device either
    for limit in (0, -5):
        got = ctypes.c_uint32(55)
        assert hip_lib.wax_hip_timeline_probe(None, None, fid.ctypes.data_as(u64), 4, limit, 1, None, 0, ids.ctypes.data_as(u64), None,
                                              ctypes.byref(got)) == 0
        assert got.value == 0 and bool(np.all(ids == 11))


def test_model_restates_the_reference_on_a_hand_case():
    """Frames 1 .. 6 as toc.frames holds them; timestamps with ties; frame 4 deleted."""
    ids = np.array([5, 1, 6, 2, 4, 3], dtype=np.uint64)           # row order is not frame order
    ts = np.array([10, 10, 30, 20, 30, 10], dtype=np.int64)
    fl = np.array([0, 0, 0, 0, ref.FLAG_DELETED, 0], dtype=np.uint32)
    assert ref.timeline_model(ts, fl, ids, 10, True, deny=ref.FLAG_DELETED)[0].tolist() == [6, 2, 1, 3, 5]
    assert ref.timeline_model(ts, fl, ids, 10, False, deny=ref.FLAG_DELETED)[0].tolist() == [1, 3, 5, 2, 6]
    assert ref.timeline_model(ts, fl, ids, 10, True)[0].tolist() == [4, 6, 2, 1, 3, 5]
    assert ref.timeline_model(ts, fl, ids, 2, False, after=10, before=30)[0].tolist() == [1, 3]
    assert ref.timeline_model(ts, fl, ids, 10, False, after=11, before=30)[0].tolist() == [2]
    assert ref.timeline_model(ts, fl, ids, 0, True)[0].size == 0 and ref.timeline_model(ts, fl, ids, -1, True)[0].size == 0
    assert ref.timeline_model(None, None, ids, 3, True)[0].tolist() == [1, 2, 3]          # no attributes: all ties


def test_case_names_are_unique_and_cover_what_the_gpu_tests_claim():
    names = [c.name for c in ref.CASES]
    assert len(set(names)) == len(names)
    assert {c.n for c in ref.CASES} == set(ref.SIZES)
    assert {c.limit for c in ref.CASES} >= set(ref.LIMITS)
    for n in ref.SIZES:
        here = [c for c in ref.CASES if c.n == n]
        assert {(c.ts_kind, c.newest) for c in here} >= {(k, o) for k in ("asc", "desc", "equal", "extremes") for o in (False, True)}
        assert any(c.id_kind == "high" for c in here) and any(c.count == 0 for c in here) and any(c.deny for c in here)
    hi = ref.columns(next(c for c in ref.CASES if c.id_kind == "high"))[2]
    assert bool((hi >= np.uint64(2**63)).any()) and bool((hi < np.uint64(2**63)).any())
    ex = ref.columns(next(c for c in ref.CASES if c.ts_kind == "extremes"))[0]
    assert set(ex.tolist()) == {ref.I64_MIN, -1, 0, ref.I64_MAX}


@pytest.mark.parametrize("case", ref.CASES, ids=lambda c: c.name)
def test_case_is_what_it_claims(case):
    ids, ts = ref.expected(case)
    assert len(ids) == len(ts) == case.count, "the claimed count is a closed form of the parameters; the model must agree"
    assert case.count <= case.limit
    if "tie" in case.tags:
        assert not np.array_equal(ids, ref.expected(case, "row")[0]), "a selection that broke ties by row would pass this case"
    if "boundary" in case.tags:
        cols = ref.columns(case)
        held = int(np.count_nonzero(cols[0] == case.after)), int(np.count_nonzero(cols[0] == case.before))
        assert min(held) > 1, "the bounds sit on timestamps several rows hold"
        for after, before in ((case.after + 1, case.before), (case.after - 1, case.before), (case.after, case.before + 1), (case.after, case.before - 1)):
            moved = ref.timeline_model(cols[0], cols[1], cols[2], case.limit, case.newest, after, before, case.deny)[0]
            assert not np.array_equal(moved, ids), (after, before)
