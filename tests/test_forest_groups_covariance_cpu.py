"""Option "forest_groups_covariance" on the CPU, under host sanitizers: which covariance pass a batch of forest windows of differing
topologies takes (localization_amd/csrc/window_dispatch.cpp: covariance_kind, cov_admitted, cov_stale, cov_switches, the keyed reuse of the
host path's tables) and the header bounds of the grouped launcher (window_layouts.h: forest_cov_groups_lds_bytes).

tests/host/forest_groups_covariance_driver.cpp (its own main; window_dispatch.cpp and window_structure.cpp compiled from source, nothing else
of the product, no HIP call) is built with g++ under AddressSanitizer + UBSan and run as a program, once per section.  The driver states its
expectations next to its calls; a non-zero exit status or anything on stderr fails the case.  That the rules are unchanged for every option
state and verdict from before the option is tests/test_window_dispatch_cpu.py's recorded grid, which this change leaves as it is."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "localization_amd", "csrc")
FLAGS = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("forest_groups_covariance_driver")
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("a sanitized program cannot be compiled and linked: no g++")
    rocm = os.path.dirname(os.path.dirname(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")))
    src = [os.path.join(ROOT, "tests", "host", "forest_groups_covariance_driver.cpp"), os.path.join(CSRC, "window_dispatch.cpp"), os.path.join(CSRC, "window_structure.cpp")]
    # (the sanitizer runtimes linked INTO the program where the compiler has them as archives, as tests/test_window_dispatch_cpu.py does)
    for extra in (["-static-libasan", "-static-libubsan"], []):
        r = subprocess.run([cxx, "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), "-I", CSRC, "-pthread", *FLAGS, *extra, *src,
                            "-o", str(d / "driver")], capture_output=True, text=True)
        if r.returncode == 0:
            break
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]
    return str(d / "driver")


# section -> the fewest expectations it states (a section that returns early would pass with fewer)
SECTIONS = {"verdicts": 96 * 10, "admission": 768 * 24, "keyed": 13, "bounds": 30}


@pytest.mark.parametrize("section", list(SECTIONS))
def test_section(driver, section):
    r = subprocess.run([driver, section], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-4000:])
    name, n, word = r.stdout.split()
    assert name == section + ":" and word == "checks" and int(n) >= SECTIONS[section], r.stdout


def test_an_unknown_section_is_an_error(driver):
    r = subprocess.run([driver, "nothing"], capture_output=True, text=True)
    assert r.returncode == 2 and "unknown section" in r.stderr
