"""The tuning table (wax_amd/csrc/tuning.inc) against tests/golden/tuning_registry.json, the record tools/tuning_snapshot.py made of
the commit before the table existed (its `k == "name"` chains), three times on one MI355X: what every settable key answers to every
probe value on an engine and on a sharded handle (part A), and what every readable key reports after a fixed workload (part B, which
catches a row wired to the wrong member and pins which keys a handle sums). The replay is the tool's own code; equality is asserted.

"store_ptr" (an address) is never compared; a part-B key whose three records disagreed is listed under "unstable" with its values and
not compared either (at most four may be). "mirror_scan_unavailable" and "mirror8_unavailable" need an allocation failure: they are
compared at the 0 this workload leaves them at."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def wax(hip_lib):
    import wax_amd
    if hip_lib.wax_hip_device_count() == 0:
        pytest.skip("no HIP device on this host: the gpu-marked tests run on the MI355X box (pytest -m gpu)")
    assert hip_lib.wax_hip_available() == 1, "a HIP device is visible but it is not gfx950: the HIP path needs an MI355X"
    return wax_amd


@pytest.fixture(scope="module")
def snapshot():
    spec = importlib.util.spec_from_file_location("tuning_snapshot", os.path.join(ROOT, "tools", "tuning_snapshot.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def registry():
    with open(os.path.join(ROOT, "tests", "golden", "tuning_registry.json")) as f:
        return json.load(f)


def test_the_record_is_a_usable_yardstick(registry):
    unstable = registry["unstable"]
    assert len(unstable["single"]) + len(unstable["sharded"]) <= 4, unstable
    single = registry["part_b"]["single"]
    for name in ("batch_multi_queries", "mirror_shared_passes", "predicate_batch_classes", "search_many_masked"):   # read by no other test
        assert single[name] > 0, name
    assert registry["part_a"]["single"].keys() == set(registry["keys"]["settable"])


def test_every_settable_key_answers_every_probe_as_recorded(wax, snapshot, registry):
    got = snapshot.part_a(wax, registry["keys"])
    want = registry["part_a"]
    assert got.keys() == want.keys()
    for side in ("single", "sharded"):
        assert got[side].keys() == want[side].keys()
        for key in sorted(want[side]):
            assert got[side][key]["fresh"] == want[side][key]["fresh"], (side, key)
            for g, w in zip(got[side][key]["probes"], want[side][key]["probes"]):   # [value, "ok" | error class, error text, getTuning after]
                assert g == w, (side, key, g, w)
            assert len(got[side][key]["probes"]) == len(want[side][key]["probes"])
    for what in ("unknown", "wrong_case", "sharded_unknown"):
        assert got[what] == want[what], what
    assert want["unknown"] == {"set": ["EncodingError", "unknown tuning key 'no_such_key'"], "get": -1}


def test_every_readable_key_after_the_workload_reads_as_recorded(wax, snapshot, registry):
    got = snapshot.part_b(wax, registry["keys"])
    for side in ("single", "sharded"):
        want = registry["part_b"][side]
        print(side, {k: (got[side][k], want.get(k, registry["unstable"][side].get(k))) for k in sorted(got[side])})
        assert set(got[side]) == set(want) | set(registry["unstable"][side])
        wrong = {k: (got[side][k], v) for k, v in want.items() if got[side][k] != v}
        assert not wrong, (side, wrong)   # key: (this tree, the record)
