"""The host rules of the sharded handle live in two headers of plain C++17 without HIP: wax_amd/csrc/shard_layout.h (where a row goes, which
rows move when the blocks double, what a reserve and a segment load ask of each shard, the bases) and shard_merge.h (G shards' sorted
answers -> one: by key, by score, timeline pairs, grouped roots). Each has a stand-alone driver with its own main under
tests/<name>/driver.cpp, which holds it to a model of ONE engine for 1 .. 9 shards; here they are compiled with g++ under AddressSanitizer
and UBSan and run. No GPU is needed and nothing is loaded into Python."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wax_amd", "csrc")
HEADERS = ("shard_layout.h", "shard_merge.h")

# every one must be entered at least once, and the driver may enter no other
REQUIRED_STATES = {
    "shard_layout": (
        "first_batch_below_the_floor_stays_in_shard_0", "min_mb_0_spreads_from_the_first_row", "one_shard_doubles_without_moves",
        "odd_shard_count_doubling", "even_shard_count_doubling", "doubling_stopped_after_every_move", "failed_doubling_then_append",
        "second_doubling_after_a_failed_one", "append_over_several_blocks", "append_after_removal_goes_to_the_tail",
        "reserve_on_an_empty_handle_adopts_the_layout", "reserve_on_a_non_empty_handle_keeps_it", "reserve_hint_sizes_the_first_rows",
        "reserve_covers_the_announced_rows", "segment_shorter_than_one_block", "segment_ends_on_a_block_edge",
        "segment_with_an_empty_tail_shard", "segment_into_a_larger_block", "block_size_rules", "random_sequences",
    ),
    "shard_merge": (
        "key_fewer_rows_than_limit", "key_pads_in_the_middle", "key_pads_inside_a_run", "key_limit_1", "key_empty_shard",
        "key_more_rows_than_limit",
        "score_ties_across_shards", "score_ties_inside_a_shard", "score_capacity_below_limit", "score_capacity_0", "score_scratch_reused",
        "timeline_newest_first", "timeline_oldest_first", "timeline_equal_timestamps_by_id", "timeline_extreme_timestamps",
        "timeline_ids_from_2_63", "timeline_capacity_below_limit", "timeline_without_timestamps_out",
        "grouped_root_in_several_shards_different_bits", "grouped_root_in_several_shards_equal_bits", "grouped_negative_bits",
        "grouped_more_roots_than_limit", "grouped_with_members", "grouped_without_members",
    ),
}
ASAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.mark.parametrize("name", sorted(REQUIRED_STATES))
def test_driver_under_address_and_ub_sanitizers(name, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp(name + "_asan") / "driver")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + ASAN +
                   ["-I" + CSRC, os.path.join(ROOT, "tests", name, "driver.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert out.stderr == "", out.stderr[-4000:]
    entered = {m.group(1): int(m.group(2)) for m in re.finditer(r"^state (\w+) (\d+)$", out.stdout, flags=re.M)}
    assert set(entered) == set(REQUIRED_STATES[name])
    assert [s for s in entered if entered[s] == 0] == []
    assert re.search(r"^ok: .*\b%d states$" % len(entered), out.stdout, flags=re.M)


def test_the_headers_are_host_only():
    """C++17 and the standard library, nothing else: that is what lets the drivers compile them with plain g++."""
    for header in HEADERS:
        src = open(os.path.join(CSRC, header)).read()
        includes = re.findall(r"#include\s+([<\"][^>\"]+[>\"])", src)
        assert includes and [i for i in includes if i.startswith('"')] == [], header
        assert not re.search(r"\bhip[A-Z_]\w*|__device__|__global__", re.sub(r"//[^\n]*", " ", src)), header


def _code_lines(name):
    for i, line in enumerate(open(os.path.join(CSRC, name)), 1):
        yield i, line.split("//", 1)[0]


def test_no_engine_file_keeps_a_copy_of_what_moved():
    """The fan-out bookkeeping is written once (sh_fan_out), the ids are routed once (sh_route), and no .inc file sorts hits by key, merges
    by score, reverses a timestamp, keeps a best-per-root map or does block arithmetic of its own."""
    gone = re.compile(r"\.key\s*<\s*\w+\.key|std::stable_sort|\bmerge_shard_results\b|\bsh_block_rows_for\b"
                      r"|\bsh_tail\b|\bsh_double_blocks\b|\bround_up64\b|->block_rows\b|->reserve_hint\b|std::map<uint64_t,\s*Best>"
                      r"|~\w*ts\b|\b(struct|class)\s+(ShardLayout|ShardAnswer|ShardHit|GroupMerge|GroupBest)\b")
    hits, finds = [], []
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith(".inc"):
            continue
        for i, code in _code_lines(name):
            if gone.search(code):
                hits.append(f"{name}:{i}: {code.strip()}")
            if name == "sharded.inc" and "sh_find(" in code:
                finds.append(code.strip())
    assert hits == []
    sh = open(os.path.join(CSRC, "sharded.inc")).read()
    # the per-shard codes and texts are kept in one place, g_last_error crosses threads there, and the workers are handed their jobs there
    assert len(re.findall(r"std::vector<std::string>\s+errs\(", sh)) == 1
    assert len(re.findall(r"errs\[g\] = g_last_error", sh)) == 1 and len(re.findall(r"workers\.(try_)?run_all\(", sh)) == 2
    # sh_find: its definition, the router, the single-id calls (add's upsert and new-id run, add_batch_device's check, remove, get_terms)
    assert len(finds) == 7, finds


def test_the_retired_functions_are_not_defined_in_sharded_inc():
    sh = re.sub(r"//[^\n]*", " ", open(os.path.join(CSRC, "sharded.inc")).read())
    for name in ("merge_shard_results", "sh_block_rows_for", "sh_tail", "sh_double_blocks"):
        assert not re.search(r"\b%s\s*\(" % name, sh), name
    for name in ("sh_fan_out", "sh_route"):
        assert len(re.findall(r"^[\w:<>\s\*]*\b%s\(ShardedState\*" % name, sh, flags=re.M)) == 1, name
    assert '#include "shard_layout.h"' in open(os.path.join(CSRC, "engine.hip")).read()
    assert '#include "shard_merge.h"' in open(os.path.join(CSRC, "engine.hip")).read()
    build = open(os.path.join(ROOT, "wax_amd", "build.py")).read()
    assert '"shard_layout.h"' in build and '"shard_merge.h"' in build
