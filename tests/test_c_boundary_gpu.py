"""tests/c_abi/consumer.cpp on the device: every public member of include/wax_hip.hpp and the host-pointer exports without a
wrapper, called from native code and compared with the program's own float64 model (tests/test_c_boundary_cpu.py holds the
program to the wrapper and proves its input conditions without a GPU). One child process, one run.

Wall time on an MI355X, measured once: the test takes 4.4 s (compile, model-only run, the checks on the device) plus 1.5 s of
session set-up; the consumer's own run is about 2 s of that."""
import subprocess

import pytest

from test_c_boundary_cpu import build_consumer, model_only_checks, tolerances


@pytest.mark.gpu
def test_native_consumer_agrees_with_its_float64_model(hip_lib, tmp_path):
    if hip_lib.wax_hip_device_count() == 0:
        pytest.skip("no HIP device on this host")
    from wax_amd import build
    exe = build_consumer(build.build(), tmp_path)
    listed = model_only_checks(exe)
    out = subprocess.run([exe] + tolerances(), capture_output=True, text=True, timeout=120)
    report = out.stdout[-20000:] + out.stderr[-4000:]
    bad = "\n".join(line for line in out.stdout.splitlines() if not line.startswith("ok "))
    assert out.returncode == 0, bad + "\n" + report
    assert f"checks {len(listed)} failed 0" in out.stdout, bad + "\n" + report
    ok = [line.split(" ", 1)[1] for line in out.stdout.splitlines() if line.startswith("ok ")]
    # the cap against hidden failures: on a GPU no check may be skipped, and none may run that the model did not vet
    assert sorted(ok) == sorted(listed), f"ok names differ from --model-only's: {sorted(set(listed) ^ set(ok))[:20]}\n" + report
