"""Option "prior_information_structured" in localization_amd/csrc/window_dispatch.cpp on the CPU: tests/host/structured_prior_dispatch_driver.cpp
(its own main; window_dispatch.cpp and window_structure.cpp compiled from source, nothing else of the product, no HIP call) is built with g++
under AddressSanitizer + UBSan and run as a program.  The driver holds pick_kernel, batch_topology's translation-only clause, covariance_kind,
cov_admitted, cov_stale and cov_switches to the rule over the full product of the switches (its header lists what it asserts); a non-zero
exit status or anything on stderr fails the test.  The recorded table of tests/test_window_dispatch_cpu.py covers the rules with the option's
fields at their defaults."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "localization_amd", "csrc")
FLAGS = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_structured_prior_rules_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("a sanitized program cannot be compiled and linked: no g++")
    rocm = os.path.dirname(os.path.dirname(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")))
    src = [os.path.join(ROOT, "tests", "host", "structured_prior_dispatch_driver.cpp"), os.path.join(CSRC, "window_dispatch.cpp"), os.path.join(CSRC, "window_structure.cpp")]
    for extra in (["-static-libasan", "-static-libubsan"], []):
        r = subprocess.run([cxx, "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), "-I", CSRC, "-pthread", *FLAGS, *extra, *src,
                            "-o", str(tmp_path / "driver")], capture_output=True, text=True)
        if r.returncode == 0:
            break
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]
    r = subprocess.run([str(tmp_path / "driver")], capture_output=True, text=True)
    print(r.stdout.strip())
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-4000:])
    assert "checks hold" in r.stdout
