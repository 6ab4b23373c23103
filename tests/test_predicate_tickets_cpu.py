"""wax_hip_search_predicate_submit / wax_hip_predicate_ticket_stats (submitFiltered / predicateTicketStats), host side: the entry
points are declared, bound and exported under the same ABI version, the read-out struct has the header's layout, NULL arguments are
refused before anything is written, and the Python wrapper checks its arguments before it reaches the library."""
import ctypes
import re

import numpy as np
import pytest

from wax_amd import _abi, engine
from wax_amd.errors import EncodingError

SUBMIT, STATS = "wax_hip_search_predicate_submit", "wax_hip_predicate_ticket_stats"
FIELDS = ("submitted", "rode", "masked_passes", "certified", "fallbacks", "deferred", "host_decided", "bitmap_builds", "bitmap_hits")


def header():
    text = open(_abi.HEADER_PATH).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


@pytest.mark.parametrize("name,nargs", [(SUBMIT, 8), (STATS, 2)])
def test_symbols_are_declared_bound_and_exported(hip_lib, name, nargs):
    assert name in _abi.declared_symbols()
    assert len(_abi.SIGNATURES[name][1]) == nargs and _abi.SIGNATURES[name][0] is ctypes.c_int
    assert hasattr(hip_lib, name)
    text, code = header()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
    assert m and len(m.group(1).split(",")) == nargs
    assert re.search(r"#define\s+WAX_HIP_ABI_VERSION\s+2\b", text)      # new functions, not a new ABI
    assert hip_lib.wax_hip_abi_version() == 2


def test_submit_signature_is_the_headers():
    _, code = header()
    flat = " ".join(code.split())
    assert ("int wax_hip_search_predicate_submit(wax_hip_engine* e, const float* query, uint32_t dims, int32_t top_k, int has_min_score, "
            "float min_score, const wax_hip_row_predicate* pred, uint64_t* out_ticket);") in flat
    assert _abi.SIGNATURES[SUBMIT][1] == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.c_uint32, ctypes.c_int32, ctypes.c_int,
                                          ctypes.c_float, ctypes.POINTER(_abi.RowPredicate), ctypes.POINTER(ctypes.c_uint64)]
    assert _abi.SIGNATURES[STATS][1] == [ctypes.c_void_p, ctypes.POINTER(_abi.PredicateTicketStats)]


def test_stats_struct_layout_matches_the_header():
    _, code = header()
    m = re.search(r"typedef\s+struct\s+wax_hip_predicate_ticket_stats_t\s*\{(.*?)\}\s*wax_hip_predicate_ticket_stats_t\s*;", code, flags=re.S)
    assert m, "the struct is not declared"
    body = m.group(1)
    assert re.fullmatch(r"\s*uint64_t\s+[a-z_,\s]+;\s*", body), body
    names = tuple(n.strip() for n in re.sub(r"uint64_t|;", "", body).split(","))
    assert names == FIELDS
    assert tuple(n for n, _ in _abi.PredicateTicketStats._fields_) == FIELDS
    assert all(t is ctypes.c_uint64 for _, t in _abi.PredicateTicketStats._fields_)
    assert ctypes.sizeof(_abi.PredicateTicketStats) == 8 * len(FIELDS)
    for i, name in enumerate(FIELDS):
        assert getattr(_abi.PredicateTicketStats, name).offset == 8 * i


def test_null_arguments_are_refused_and_outputs_untouched(hip_lib):
    f32 = ctypes.POINTER(ctypes.c_float)
    q = np.zeros(8, np.float32)
    pred = _abi.RowPredicate(0, 0, 0, 0, 7)
    ticket = ctypes.c_uint64(77)
    rc = getattr(hip_lib, SUBMIT)(None, q.ctypes.data_as(f32), 8, 10, 0, 0.0, ctypes.byref(pred), ctypes.byref(ticket))
    assert rc == _abi.ERR_INVALID_ARGUMENT and "null" in _abi.last_error()
    assert ticket.value == 77
    rc = getattr(hip_lib, SUBMIT)(None, None, 8, 10, 1, 0.5, None, None)
    assert rc == _abi.ERR_INVALID_ARGUMENT and "null" in _abi.last_error()
    st = _abi.PredicateTicketStats(*([5] * len(FIELDS)))
    rc = getattr(hip_lib, STATS)(None, ctypes.byref(st))
    assert rc == _abi.ERR_INVALID_ARGUMENT and "null" in _abi.last_error()
    assert all(getattr(st, name) == 5 for name in FIELDS)


def test_wrapper_checks_its_arguments():
    p = engine.ticket_predicate()
    assert (p.has_after, p.after, p.has_before, p.before, p.deny_flags) == (0, 0, 0, 0, 0)
    p = engine.ticket_predicate((None, 9), 0b101)
    assert (p.has_after, p.after, p.has_before, p.before, p.deny_flags) == (0, 0, 1, 9, 5)
    p = engine.ticket_predicate((-3, None), 0xffffffff)
    assert (p.has_after, p.after, p.has_before, p.before, p.deny_flags) == (1, -3, 0, 0, 0xffffffff)
    p = engine.ticket_predicate([np.int64(4), 2 ** 63 - 1], np.uint32(1 << 8))
    assert (p.has_after, p.after, p.has_before, p.before, p.deny_flags) == (1, 4, 1, 2 ** 63 - 1, 256)
    for bad in (5, (1,), (1, 2, 3), "ab"):
        with pytest.raises(EncodingError, match="timeRange"):
            engine.ticket_predicate(bad, 0)
    for bad in ((1.5, None), (None, "x"), (2 ** 63, None)):
        with pytest.raises(EncodingError, match="timeRange bound"):
            engine.ticket_predicate(bad, 0)
    for bad in (-1, 1 << 32, 1.0, None):
        with pytest.raises(EncodingError, match="denyFlags"):
            engine.ticket_predicate(None, bad)


def test_python_methods_exist():
    import wax_amd
    assert callable(wax_amd.HIPVectorEngine.submitFiltered) and callable(wax_amd.HIPVectorEngine.predicateTicketStats)
