"""wax_amd/csrc/derived_rows.h holds how far the bf16 mirror, the 8-bit code mirror and the id -> row table have followed the store: one
small state machine each, one operation per mutation of the store, in plain C++ without HIP. tests/derived_rows/driver.cpp replays
seeded random mutation sequences on it against a naive model and three device shadows that only receive what a reader is told to build;
here it is compiled as a stand-alone program under AddressSanitizer and UBSan and run. No GPU is needed and nothing is loaded into Python."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wax_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "derived_rows", "driver.cpp")

# the mirror's entries of store_sequence_ref.MIRROR_CLASSES where they exist, and what only the header's driver can reach: every one
# must be entered (the cap states at a cap of 8 in the random sequences, the real_cap ones once at kMirrorMaxDirty)
REQUIRED_STATES = (
    "upsert_converted", "upsert_above_fill", "upsert_while_restarting",
    "upserts_cap_listed", "upserts_cap_plus_one_restart", "real_cap_listed", "real_cap_plus_one_restart",
    "remove_below_fill", "remove_dirty_below", "remove_dirty_above", "remove_dirty_at", "remove_above_fill", "remove_not_followed",
    "remove_batch_straddle", "remove_batch_dirty_removed", "remove_batch_dirty_surviving", "remove_batch_tail_only",
    "remove_batch_not_followed", "remove_batch_above_fill",
    "growth_dirty_pending", "growth_unconverted_pending", "growth_restarts_codes", "growth_restarts_idtable",
    "append_after_settle", "replaced_with_dirty_pending", "lost_then_read",
    "wanted_third_request_builds", "wanted_reset_by_mutation", "reader_finds_everything_current",
)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("derived_rows") / "driver")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + CSRC, DRIVER, "-o", exe], check=True)
    return exe


def test_fills_follow_the_model_and_the_shadows_follow_the_fills(driver):
    out = subprocess.run([driver], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert out.stderr == "", out.stderr[-4000:]
    entered = {m.group(1): int(m.group(2)) for m in re.finditer(r"^state (\w+) (\d+)$", out.stdout, flags=re.M)}
    assert set(REQUIRED_STATES) <= set(entered)
    assert [s for s in entered if entered[s] == 0] == []
    assert re.search(r"^ok: \d+ sequences of \d+ operations, %d states$" % len(entered), out.stdout, flags=re.M)


def test_the_header_is_host_only():
    """C++17 and the standard library, nothing else: that is what lets the driver compile it with plain g++."""
    src = open(os.path.join(CSRC, "derived_rows.h")).read()
    includes = re.findall(r"#include\s+([<\"][^>\"]+[>\"])", src)
    assert includes and [i for i in includes if i.startswith('"')] == []
    assert not re.search(r"\bhip[A-Z_]\w*|__device__|__global__|\bmutex\b", re.sub(r"//[^\n]*", " ", src))


def test_no_engine_file_keeps_a_fill_of_its_own():
    """The engine's files go through DerivedRows: none of them names a retired field or hook."""
    gone = re.compile(r"\bmirror_note_\w+|\bc8_note_\w+|\b(mirror_valid|c8_valid|c8_stale|rows8|n_dirty|mirror_wanted|c8_wanted)\b"
                      r"|\.dirty\b|\bidhash\.(valid|stale|rows)\b|\bbatch\.(stale|rows)\b")
    hits = []
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith(".inc"):
            continue
        for i, line in enumerate(open(os.path.join(CSRC, name)), 1):
            if gone.search(line.split("//", 1)[0]):
                hits.append(f"{name}:{i}: {line.strip()}")
    assert hits == []
