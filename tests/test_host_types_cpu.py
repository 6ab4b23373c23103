"""The engine's host-side concurrency lives in four headers of plain C++17 without HIP: wax_amd/csrc/work_pool.h (the pools of per-call
workspaces and the ticket tables), rw_lock.h (the reader/writer lock and the tickets per submitting thread), shard_workers.h (the hand-off
to the per-shard threads) and id_map.h (frame id -> row). Each has a stand-alone driver with its own main under tests/<name>/driver.cpp;
here they are compiled with g++ under AddressSanitizer and UBSan and run, and the threaded ones a second time under ThreadSanitizer.
No GPU is needed and nothing is loaded into Python."""
import os
import platform
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wax_amd", "csrc")
HEADERS = ("work_pool.h", "rw_lock.h", "shard_workers.h", "id_map.h")

# every one must be entered at least once, and the driver may enter no other
REQUIRED_STATES = {
    "work_pool": (
        "reuse", "fresh_below_cap", "wait_woken_by_release", "try_refused", "holder_grows", "holder_refused_at_hard_cap",
        "make_fails_nothing_registered", "cap_raised_wakes_waiter", "cap_lowered_below_size", "for_each_sees_every_item_once",
        "deadlock_grow_both_return", "deadlock_try_both_refused", "threads_contended_wait",
        "ticket_ids_from_one", "ticket_taken_once_from_any_thread", "ticket_unknown_refused", "ticket_peek_leaves_it",
    ),
    "rw_lock": (
        "holder_reenters_past_queued_writer", "reader_without_ticket_queues_behind_writer", "writer_excludes_readers",
        "unlock_from_another_thread", "epoch_constant_under_shared_lock", "epoch_advances_by_one_per_writer",
        "holding_drops_when_another_thread_collects", "reader_waits_for_active_writer", "threads_mixed",
    ),
    "shard_workers": (
        "burst_workers_polling", "pause_workers_asleep", "long_job_caller_sleeps", "three_callers_at_once",
        "try_refused_while_long_job_runs", "try_runs_when_free", "stop_while_asleep", "stop_while_polling", "stop_before_any_job",
        "on_start_once_per_worker",
    ),
    "id_map": (
        "overwrite_present", "growth_and_rehash", "erase_absent", "erase_cluster_head", "erase_cluster_middle", "erase_cluster_tail",
        "wrap_erase_before_the_end", "wrap_erase_after_the_start", "wrap_mixed_homes", "reserve_spares_growth", "clear_empties",
        "renumber_first_on_word_boundary", "renumber_first_off_word_boundary", "renumber_last_row", "renumber_single_row",
        "renumber_whole_word", "renumber_three_words_one_empty", "renumber_nothing", "erase_row_renumbers", "store_of_100000_rows",
    ),
}
THREADED = ("work_pool", "rw_lock", "shard_workers")
ASAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
TSAN = ["-fsanitize=thread", "-O1", "-g"]


def _build(tmp_path_factory, name, flags, tag):
    exe = str(tmp_path_factory.mktemp(name + "_" + tag) / "driver")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pthread"] + flags +
                   ["-I" + CSRC, os.path.join(ROOT, "tests", name, "driver.cpp"), "-o", exe], check=True)
    return exe


def _entered_all(name, out):
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert out.stderr == "", out.stderr[-4000:]
    entered = {m.group(1): int(m.group(2)) for m in re.finditer(r"^state (\w+) (\d+)$", out.stdout, flags=re.M)}
    assert set(entered) == set(REQUIRED_STATES[name])
    assert [s for s in entered if entered[s] == 0] == []
    assert re.search(r"^ok: .*\b%d states$" % len(entered), out.stdout, flags=re.M)


@pytest.mark.parametrize("name", sorted(REQUIRED_STATES))
def test_driver_under_address_and_ub_sanitizers(name, tmp_path_factory):
    exe = _build(tmp_path_factory, name, ASAN, "asan")
    _entered_all(name, subprocess.run([exe], capture_output=True, text=True, timeout=120))


@pytest.mark.parametrize("name", THREADED)
def test_threaded_driver_under_thread_sanitizer(name, tmp_path_factory):
    exe = _build(tmp_path_factory, name, TSAN, "tsan")
    # ThreadSanitizer maps its shadow at fixed addresses, and where the kernel randomises a program's own mappings widely its start-up
    # meets one of them there (it then ends with "unexpected memory mapping", or dies before it can say so). Without that randomisation it
    # starts, so the driver is first run that way; where setarch is missing or may not set the personality, it is run as it is.
    out = None
    if shutil.which("setarch"):
        out = subprocess.run(["setarch", platform.machine(), "-R", exe], capture_output=True, text=True, timeout=240)
    if out is None or (out.stdout == "" and out.returncode != 0):
        out = subprocess.run([exe], capture_output=True, text=True, timeout=240)
    if out.stdout == "" and out.returncode != 0 and "unexpected memory mapping" in out.stderr:
        pytest.skip("ThreadSanitizer's runtime refused to start in this environment (\"unexpected memory mapping\") before the driver's "
                    "first line; the AddressSanitizer and UBSan build of the same driver ran")
    _entered_all(name, out)


def test_the_headers_are_host_only():
    """C++17 and the standard library, nothing else: that is what lets the drivers compile them with plain g++."""
    for header in HEADERS:
        src = open(os.path.join(CSRC, header)).read()
        includes = re.findall(r"#include\s+([<\"][^>\"]+[>\"])", src)
        assert includes and [i for i in includes if i.startswith('"')] == [], header
        assert not re.search(r"\bhip[A-Z_]\w*|__device__|__global__", re.sub(r"//[^\n]*", " ", src)), header


def test_no_engine_file_keeps_a_pool_a_ticket_map_or_a_holder_count_of_its_own():
    """The engine's files go through WorkPool, TicketTable and TicketHolders: none of them names a retired field, one of the ten retired
    acquire / release functions or the retired hooks of the holder count, and none defines a class that moved to a header."""
    gone = re.compile(r"\b(slot_mu|slot_cv|all_slots|free_slots|max_slots|slots_all|slots_free|bticket_mu|next_ticket|next_bticket|out_mu)\b|(->|\.)outstanding\b"
                      r"|\bbctx_(mu|cv|all|free|max)\b|\bfilter_(mu|cv|all|free|max)\b|\bbw_(mu|cv|all|free|max)\b"
                      r"|\b(sh_)?(acquire|release)_(slot|bctx|bwork|filter_work)\b|\bnote_(submit|collect)_id\b"
                      r"|\b(class|struct)\s+(RWLock|WriteGuard|IdMap|ShardWorkers)\b")
    hits = []
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith(".inc"):
            continue
        for i, line in enumerate(open(os.path.join(CSRC, name)), 1):
            if gone.search(line.split("//", 1)[0]):
                hits.append(f"{name}:{i}: {line.strip()}")
    assert hits == []
