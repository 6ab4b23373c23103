"""include/wax_hip.h and include/wax_hip.hpp are the drop-in boundary; wax_amd/_abi.py is a hand-written restatement of the header
that every GPU test goes through. These tests hold the restatement to what a C compiler makes of the header — struct layouts,
constants, every prototype argument by argument — and hold tests/c_abi/consumer.cpp, the native consumer with its own float64
model, to the wrapper: every public name of wax_hip.hpp must be called there. No GPU is needed: the consumer's --model-only mode
proves the gap and filter conditions of its committed seed, and without a device its default mode reports `no-device`."""
import ctypes
import os
import re
import subprocess

import pytest

import helpers
from wax_amd import _abi
from wax_amd import vector_metric

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
C_ABI = os.path.join(ROOT, "tests", "c_abi")

# header struct -> its ctypes restatement
STRUCTS = {
    "wax_hip_hit": _abi.Hit,
    "wax_hip_stats_t": _abi.Stats,
    "wax_hip_rrf_lane": _abi.RrfLane,
    "wax_hip_row_predicate": _abi.RowPredicate,
    "wax_hip_predicate_ticket_stats_t": _abi.PredicateTicketStats,
    "wax_hip_group_stats_t": _abi.GroupStats,
    "wax_hip_term_stats_t": _abi.TermStats,
    "wax_hip_term_batch_stats_t": _abi.TermBatchStats,
}

# header constant -> the Python value that restates it
CONSTANTS = {
    "WAX_HIP_OK": _abi.OK,
    "WAX_HIP_ERR_DIM_MISMATCH": _abi.ERR_DIM_MISMATCH,
    "WAX_HIP_ERR_CAPACITY": _abi.ERR_CAPACITY,
    "WAX_HIP_ERR_NO_DEVICE": _abi.ERR_NO_DEVICE,
    "WAX_HIP_ERR_ALLOC": _abi.ERR_ALLOC,
    "WAX_HIP_ERR_BAD_SEGMENT": _abi.ERR_BAD_SEGMENT,
    "WAX_HIP_ERR_METRIC_UNSUPPORTED": _abi.ERR_METRIC_UNSUPPORTED,
    "WAX_HIP_ERR_INVALID_ARGUMENT": _abi.ERR_INVALID_ARGUMENT,
    "WAX_HIP_ERR_INTERNAL": _abi.ERR_INTERNAL,
    "WAX_HIP_METRIC_COSINE": int(vector_metric.VectorMetric.cosine),
    "WAX_HIP_METRIC_DOT": int(vector_metric.VectorMetric.dot),
    "WAX_HIP_METRIC_L2": int(vector_metric.VectorMetric.l2),
    "WAX_HIP_MAX_RESULTS": _abi.MAX_RESULTS,
    "WAX_HIP_FLAG_DELETED": _abi.FLAG_DELETED,
    "WAX_HIP_FLAG_SUPERSEDED": _abi.FLAG_SUPERSEDED,
    "WAX_HIP_FLAG_SURROGATE": _abi.FLAG_SURROGATE,
    "WAX_HIP_FLAG_USER_SHIFT": _abi.FLAG_USER_SHIFT,
    "WAX_HIP_GROUP_MAX_LIMIT": _abi.GROUP_MAX_LIMIT,
    "WAX_HIP_GROUP_MAX_MEMBERS": _abi.GROUP_MAX_MEMBERS,
    "WAX_HIP_TERMS_MAX_PER_ROW": _abi.TERMS_MAX_PER_ROW,
    "WAX_HIP_TERMS_MAX_REQUIRED": _abi.TERMS_MAX_REQUIRED,
    "WAX_HIP_NO_ALLOW_LIST": _abi.NO_ALLOW_LIST,
    "WAX_HIP_NO_PARENT": _abi.NO_PARENT,
}


def build_consumer(lib_path, out_dir):
    """tests/c_abi/consumer.cpp compiled and linked as a C++ host would: the two headers, the library, an rpath."""
    exe = os.path.join(str(out_dir), "c_boundary_consumer")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + INCLUDE, os.path.join(C_ABI, "consumer.cpp"),
                    "-L" + os.path.dirname(lib_path), "-lwaxhip", "-Wl,-rpath," + os.path.dirname(lib_path), "-o", exe], check=True)
    return exe


def tolerances():
    return [repr(helpers.SCORE_TOL), repr(helpers.TIE_TOL)]


def model_only_checks(exe):
    """The names of the checks, as --model-only lists them after proving the input conditions."""
    out = subprocess.run([exe, "--model-only"] + tolerances(), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr
    names = [line.split(" ", 1)[1] for line in out.stdout.splitlines() if line.startswith("check ")]
    assert names and len(names) == len(set(names)), "check names must be unique"
    assert f"model ok: {len(names)} checks" in out.stdout
    return names


# ---- layout and constants ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("layout") / "layout")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + INCLUDE, os.path.join(C_ABI, "layout.c"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    structs, fields, consts = {}, {}, {}
    for line in out.splitlines():
        kind, *rest = line.split()
        if kind == "struct":
            structs[rest[0]] = int(rest[1])
        elif kind == "field":
            fields.setdefault(rest[0], []).append((rest[1], int(rest[2]), int(rest[3])))
        elif kind == "const":
            consts[rest[0]] = int(rest[1])
    return structs, fields, consts


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def _header_text():
    return _strip_comments(open(_abi.HEADER_PATH).read())


def test_layout_program_covers_every_struct_and_member_of_the_header(layout):
    """layout.c is written by hand: a struct or member added to the header without a line there must not go unnoticed."""
    structs, fields, _ = layout
    declared = {}
    for body, name in re.findall(r"typedef\s+struct\s+\w+\s*\{(.*?)\}\s*(\w+)\s*;", _header_text(), flags=re.S):
        members = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                first, *more = decl.split(",")
                members.append(re.findall(r"\w+", first)[-1])
                members += [m.strip().lstrip("*").strip() for m in more]
        declared[name] = members
    assert set(declared) == set(STRUCTS) == set(structs)
    for name, members in declared.items():
        assert [f[0] for f in fields[name]] == members, name


@pytest.mark.parametrize("name", sorted(STRUCTS))
def test_ctypes_structure_matches_the_compiled_layout(layout, name):
    structs, fields, _ = layout
    cls = STRUCTS[name]
    assert ctypes.sizeof(cls) == structs[name], f"{name}: sizeof"
    got = [(fname, getattr(cls, fname).offset, getattr(cls, fname).size) for fname, _ in cls._fields_]
    assert got == fields[name], f"{name}: (member, offset, size) in _abi against the C compiler"


def test_constants_match_the_compiled_header(layout, hip_lib):
    _, _, consts = layout
    for name, value in CONSTANTS.items():
        assert consts[name] == value, name
    assert consts["WAX_HIP_ABI_VERSION"] == hip_lib.wax_hip_abi_version()
    assert set(consts) == set(CONSTANTS) | {"WAX_HIP_ABI_VERSION"}
    assert _abi.ID_PAD == consts["WAX_HIP_NO_PARENT"] and _abi.KEY_PAD == (1 << 63) - 1


# ---- prototypes ---------------------------------------------------------------------------------------------------------

# C base type -> ABI class: ("int", bytes, signed) | ("float",) | ("double",) | ("void",) | ("struct", name)
_BASE = {
    "int": ("int", 4, True), "int32_t": ("int", 4, True), "uint32_t": ("int", 4, False), "int64_t": ("int", 8, True),
    "uint64_t": ("int", 8, False), "uint8_t": ("int", 1, False), "char": ("int", 1, True), "size_t": ("int", ctypes.sizeof(ctypes.c_size_t), False),
    "float": ("float",), "double": ("double",), "void": ("void",), "wax_hip_engine": ("struct", "wax_hip_engine"),
}
_BASE.update({name: ("struct", name) for name in STRUCTS})


def _c_type(decl, with_name):
    """`const uint64_t* const* lists` -> ("ptr", ("ptr", ("int", 8, False))): the ABI class of a declarator."""
    decl = decl.strip()
    depth = decl.count("*")
    words = [w for w in re.findall(r"\w+", decl) if w not in ("const", "struct")]
    if with_name and len(words) == 2:
        words = words[:1]
    assert len(words) == 1 and words[0] in _BASE, f"cannot parse the type of {decl!r}"
    t = _BASE[words[0]]
    for _ in range(depth):
        t = ("ptr", t)
    return t


def header_prototypes():
    """name -> (return class, [argument classes]) for every function include/wax_hip.h declares."""
    text = _header_text()
    text = "\n".join(line for line in text.splitlines() if not line.lstrip().startswith("#"))
    text = re.sub(r"typedef\s+(struct|enum)\s+\w+\s*\{.*?\}\s*\w+\s*;", " ", text, flags=re.S)
    text = re.sub(r"typedef\s+struct\s+\w+\s+\w+\s*;", " ", text)
    text = re.sub(r'extern\s+"C"\s*\{', " ", text).replace("}", " ")
    protos = {}
    for stmt in text.split(";"):
        stmt = " ".join(stmt.split())
        if not stmt:
            continue
        m = re.fullmatch(r"(.+?)\b(wax_hip_\w+)\s*\((.*)\)", stmt)
        assert m, f"not a prototype: {stmt!r}"
        ret, name, args = m.groups()
        arg_list = [] if args.strip() == "void" else [_c_type(a, True) for a in args.split(",")]
        assert name not in protos, name
        protos[name] = (_c_type(ret, False), arg_list)
    return protos


_STRUCT_OF = {cls: name for name, cls in STRUCTS.items()}


def _matches(ct, c):
    """Does the ctypes type `ct` describe the C ABI class `c`? c_void_p stands for any pointer; POINTER(T) also fixes the pointee."""
    if ct is None:
        return c == ("void",)
    if ct is ctypes.c_void_p:
        return c[0] == "ptr"
    if ct is ctypes.c_char_p:
        return c[0] == "ptr" and c[1][0] == "int" and c[1][1] == 1
    if isinstance(ct, type) and issubclass(ct, ctypes._Pointer):
        return c[0] == "ptr" and _matches(ct._type_, c[1])
    if isinstance(ct, type) and issubclass(ct, ctypes.Structure):
        return c == ("struct", _STRUCT_OF[ct])
    code = ct._type_
    if code == "f":
        return c == ("float",)
    if code == "d":
        return c == ("double",)
    assert code in "bBhHiIlLqQ", f"unexpected ctypes type {ct}"
    return c == ("int", ctypes.sizeof(ct), code.islower())


def test_every_prototype_of_the_header_matches_abi_signatures():
    protos = header_prototypes()
    assert sorted(protos) == _abi.declared_symbols() == sorted(_abi.SIGNATURES), "the parser, the header and _abi name the same functions"
    wrong = []
    for name, (ret, args) in sorted(protos.items()):
        restype, argtypes = _abi.SIGNATURES[name]
        if not _matches(restype, ret):
            wrong.append(f"{name}: returns {ret}, _abi says {restype}")
        if len(argtypes) != len(args):
            wrong.append(f"{name}: {len(args)} arguments, _abi lists {len(argtypes)}")
            continue
        for i, (ct, c) in enumerate(zip(argtypes, args)):
            if not _matches(ct, c):
                wrong.append(f"{name}: argument {i} is {c}, _abi says {ct}")
    assert not wrong, "\n".join(wrong)


def test_the_signature_matcher_tells_widths_signs_and_pointees_apart():
    """The comparison above is only worth something if it can fail: one wrong width, sign, pointee or struct each."""
    u64p = ("ptr", ("int", 8, False))
    assert _matches(ctypes.POINTER(ctypes.c_uint64), u64p) and _matches(ctypes.c_void_p, u64p)
    assert not _matches(ctypes.POINTER(ctypes.c_uint32), u64p) and not _matches(ctypes.POINTER(ctypes.c_int64), u64p)
    assert not _matches(ctypes.c_uint64, u64p) and not _matches(ctypes.c_void_p, ("int", 8, False))
    assert _matches(ctypes.c_int32, ("int", 4, True)) and not _matches(ctypes.c_uint32, ("int", 4, True))
    assert not _matches(ctypes.c_int64, ("int", 4, True)) and not _matches(ctypes.c_float, ("double",))
    assert _matches(ctypes.POINTER(_abi.Hit), ("ptr", ("struct", "wax_hip_hit")))
    assert not _matches(ctypes.POINTER(_abi.Hit), ("ptr", ("struct", "wax_hip_row_predicate")))
    assert _matches(ctypes.POINTER(ctypes.c_void_p), ("ptr", u64p)) and not _matches(ctypes.POINTER(ctypes.c_void_p), u64p)
    assert _c_type("const uint64_t* const* lists", True) == ("ptr", u64p) and _c_type("const char*", False) == ("ptr", ("int", 1, True))


# ---- the native consumer ------------------------------------------------------------------------------------------------

def _block(text, open_at):
    """The text between the brace at `open_at` and its partner."""
    depth = 0
    for i in range(open_at, len(text)):
        depth += text[i] == "{"
        depth -= text[i] == "}"
        if depth == 0:
            return text[open_at + 1:i], i + 1
    raise AssertionError("unbalanced braces")


def _declared_functions(text):
    """Names followed by a parameter list at brace depth 0 and parenthesis depth 0 of `text`."""
    while re.search(r"\{[^{}]*\}", text):
        text = re.sub(r"\{[^{}]*\}", " ", text)
    while re.search(r"\([^()]+\)", text):
        text = re.sub(r"\([^()]+\)", "()", text)
    return set(re.findall(r"\b(\w+)\s*\(\)", text))


def wrapper_public_names():
    """(members of wax_hip::VectorEngine's public part, free functions of namespace wax_hip) as wax_hip.hpp declares them."""
    text = _strip_comments(open(os.path.join(INCLUDE, "wax_hip.hpp")).read())
    text = "\n".join(line for line in text.splitlines() if not line.lstrip().startswith("#"))
    ns, _ = _block(text, text.index("{", text.index("namespace wax_hip")))
    at = ns.index("class VectorEngine")
    body, end = _block(ns, ns.index("{", at))
    public = body[body.index("public:") + len("public:"):body.index("private:")]
    members = _declared_functions(public)
    free = _declared_functions(ns[:at] + ns[end:])
    return members, free


def test_every_public_name_of_the_wrapper_is_called_by_the_consumer():
    members, free = wrapper_public_names()
    # the parser sees what is there: spot checks from both ends of the class and the namespace
    assert {"isAvailable", "VectorEngine", "search", "searchGrouped", "timeline", "getAttributes", "getParents", "groupStats", "reserve",
            "termBatchStats", "raw"} <= members and len(members) >= 31
    assert free == {"check", "searchMany", "searchManyFiltered"}
    src = _strip_comments(open(os.path.join(C_ABI, "consumer.cpp")).read())
    missing = []
    for name in sorted(members):
        if name == "VectorEngine":
            called = re.search(r"\bnew VectorEngine\s*\(", src) and re.search(r"\bVectorEngine\s+\w+\(", src)
        elif name == "isAvailable":
            called = re.search(r"\bVectorEngine::isAvailable\s*\(", src)
        else:
            called = re.search(r"(->|\.)" + name + r"\s*\(", src)
        if not called:
            missing.append(name)
    missing += [name for name in sorted(free) if not re.search(r"\bwax_hip::" + name + r"\s*\(", src)]
    assert not missing, f"wax_hip.hpp names without a native check in tests/c_abi/consumer.cpp: {missing}"


def test_consumer_calls_the_host_pointer_exports_that_have_no_wrapper():
    src = _strip_comments(open(os.path.join(C_ABI, "consumer.cpp")).read())
    for name in ("wax_hip_search_submit", "wax_hip_search_collect", "wax_hip_search_batch", "wax_hip_search_batch_hits",
                 "wax_hip_hits_to_results", "wax_hip_search_predicate_submit", "wax_hip_predicate_ticket_stats", "wax_hip_rrf_fuse",
                 "wax_hip_reserve", "wax_hip_stats", "wax_hip_set_tuning", "wax_hip_get_tuning", "wax_hip_metric_of", "wax_hip_device_of",
                 "wax_hip_engine_create_sharded", "wax_hip_shard_count", "wax_hip_shard_info"):
        assert re.search(r"\b" + name + r"\s*\(", src), name
    assert "#include \"wax_hip.hpp\"" in src
    includes = re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", src)
    assert [i for i in includes if "/" in i or i.endswith(".h")] == [], "the standard library and wax_hip.hpp only"
    assert not re.search(r"\b(1e-5|2e-5|0\.00001|0\.00002)\b", src), "the tolerances come from the command line"


@pytest.fixture(scope="module")
def consumer(hip_lib, tmp_path_factory):
    from wax_amd import build
    return build_consumer(build.build(), tmp_path_factory.mktemp("consumer"))


def test_model_only_proves_the_input_conditions_and_lists_the_checks(consumer):
    names = model_only_checks(consumer)
    members, free = wrapper_public_names()
    for store in ("d64.cosine", "d64.dot", "d64.l2", "d20.cosine", "d20.dot", "d20.l2"):
        mine = [n for n in names if n.startswith(store + ".")]
        assert len(mine) > 100, store
        for stage in ("after_removeBatch", "after_remove", "after_add", "after_applyPutEmbeddings", "second"):
            for kind in ("search", "searchFiltered", "searchPredicate", "searchTerms", "searchBatchFiltered", "searchBatchPredicate",
                         "searchBatchTerms", "searchGrouped", "timeline"):
                assert f"{store}.{stage}.{kind}" in mine
    assert {"many.searchMany", "many.searchManyFiltered.preds", "rrf.fuse"} <= set(names)


def test_model_only_rejects_a_tolerance_its_inputs_cannot_meet(consumer):
    """The gap condition is asserted, not assumed: with a tie tolerance far above the spacing of the scores the program refuses."""
    out = subprocess.run([consumer, "--model-only", repr(helpers.SCORE_TOL), "0.5"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 3 and "input condition violated" in out.stdout


def test_consumer_without_a_device_fails_loudly(consumer, hip_lib):
    if hip_lib.wax_hip_available():
        pytest.skip("GPU present: tests/test_c_boundary_gpu.py runs the checks")
    out = subprocess.run([consumer] + tolerances(), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("no-device: ") and "ok " not in out.stdout
