"""wax_amd/csrc/row_columns.h holds everything about the per-row columns (timestamps, flags, parents, term sets, the group slots and the
upload marks of their device copies) that lives in host memory, in plain C++ without HIP. tests/row_columns/driver.cpp replays seeded
random mutation sequences on it against a naive model and a device shadow that only receives the rows a mark asks for; here it is
compiled as a stand-alone program under AddressSanitizer and UBSan and run. No GPU is needed and nothing is loaded into Python."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wax_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "row_columns", "driver.cpp")

# the host-side entries of store_sequence_ref.COLUMN_CLASSES and the moves between two stores: every one must be entered
REQUIRED_STATES = (
    "attrs_first_set", "attrs_set_behind_column", "parents_first_set", "parents_set_behind_column", "terms_first_set", "terms_set_behind_column",
    "attrs_remove_below_column", "attrs_remove_behind_column", "attrs_remove_batch_straddles_column_end",
    "parents_remove_below_column", "parents_remove_behind_column", "parents_remove_batch_straddles_column_end",
    "terms_remove_below_column", "terms_remove_behind_column", "terms_remove_batch_straddles_column_end",
    "attrs_emptied", "parents_emptied", "terms_emptied",
    "terms_same_size_overwrite", "terms_resize_rebuild", "terms_all_sets_empty", "parents_renumber_from_scratch", "three_columns_different_lengths",
    "move_into_store_without_columns", "move_into_columns_ending_below_dst_before", "move_from_store_without_columns", "truncate_after_partial_move",
    "move_onto_rows_a_device_copy_holds",
)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("row_columns") / "driver")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, DRIVER, "-o", exe], check=True)
    return exe


def test_columns_follow_the_model_and_the_shadow_follows_the_marks(driver):
    out = subprocess.run([driver], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert out.stderr == "", out.stderr[-4000:]
    entered = {m.group(1): int(m.group(2)) for m in re.finditer(r"^state (\w+) (\d+)$", out.stdout, flags=re.M)}
    assert set(REQUIRED_STATES) <= set(entered)
    assert [s for s in entered if entered[s] == 0] == []
    assert re.search(r"^ok: \d+ sequences of \d+ operations, %d states$" % len(entered), out.stdout, flags=re.M)


def test_the_header_is_host_only():
    """C++17, the standard library and include/wax_hip.h, nothing else: that is what lets the driver compile it with plain g++."""
    src = open(os.path.join(CSRC, "row_columns.h")).read()
    includes = re.findall(r"#include\s+([<\"][^>\"]+[>\"])", src)
    assert [i for i in includes if i.startswith('"')] == ['"wax_hip.h"']
    assert not re.search(r"\bhip[A-Z_]\w*|__device__|__global__", re.sub(r"//[^\n]*", " ", src))


def test_no_engine_file_reaches_into_a_column_or_a_mark():
    """The engine's files go through RowColumns: none of them names a column's vectors or a mark's two numbers."""
    gone = re.compile(r"\b(attr_ts|attr_flags|attr_parent|term_off|term_val|grp_slot|grp_slot_of|grp_slot_root|grp_rows|\w+_stale_from|\w+_dev_rows"
                      r"|attr_note_\w+|parent_note_\w+|term_note_\w+)\b")
    hits = []
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith(".inc"):
            continue
        for i, line in enumerate(open(os.path.join(CSRC, name)), 1):
            code = line.split("//", 1)[0]
            code = re.sub(r"\bsp\.term_(off|val)\b", " ", code)          # (RowListPred's fields: the device pointers a kernel takes)
            if gone.search(code):
                hits.append(f"{name}:{i}: {line.strip()}")
    assert hits == []
