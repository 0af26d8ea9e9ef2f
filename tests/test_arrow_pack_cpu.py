"""The arrowhead rule for ONE window (localization_amd/csrc/arrow_pack.h; DESIGN.md §2, "Upload from device arrays") without a GPU.
arrow_window_structure and arrow_window_pack — what window_structure_kernel.hip restates lane-parallel — run window by window through the
stand-alone driver tests/host/arrow_pack_driver.cpp (g++, AddressSanitizer + UBSan; every window's tables at exactly the size its counts
name), which merges them and holds the result to build_arrow_aux on the same batch: verdict, hdr, rslot, rec and prec byte for byte, and
every size.  The driver exits with 1 on any difference.  Here its verdicts, the refusal it names and the border it finds are also held to
tests/_window_structure_model.py and to what the batches were built for (build_arrow_aux's tables themselves are held to that model by
tests/test_window_structure_cpu.py)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _window_structure_model as M
import test_window_structure_cpu as W
from _window_structure_model import Batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "localization_amd", "csrc")
OK, ANCHOR_CODE, BORDER, CHAIN_GAP, PAIR_TWICE, SELF_RANGE = range(6)       # arrow_pack.h: ArrowRefusal
BATCH_SIZES, BATCH_LDS = 1, 2                                                # the driver's batch-level refusal


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("arrow_pack_driver")
    cxx = shutil.which("g++")
    assert cxx is not None, "g++ is needed to build tests/host/arrow_pack_driver.cpp (the project's build() needs it as well)"
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    rocm = os.path.dirname(os.path.dirname(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")))
    src = [os.path.join(ROOT, "tests", "host", "arrow_pack_driver.cpp"), os.path.join(CSRC, "window_structure.cpp")]
    logs = []
    for extra in (["-static-libasan", "-static-libubsan"], []):   # (the runtimes as archives where the compiler has them)
        r = subprocess.run([cxx, "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), "-I", CSRC, "-pthread", *flags, *extra, *src,
                            "-o", str(d / "driver")], capture_output=True, text=True)
        logs.append(" ".join(extra) + ": " + r.stderr[-1500:])
        if r.returncode == 0:
            return str(d / "driver")
    raise AssertionError("\n".join(logs))


def run(driver, tmp_path, batches):
    path = tmp_path / "in.bin"
    with open(path, "wb") as f:
        for b in batches:
            b.write(f)
    r = subprocess.run([driver, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-3000:])
    names = ("verdict", "first", "code", "batch", "nb_max", "jmax", "jpmax", "list_cap")
    out = [dict(zip(names, (int(x) for x in line.split()))) for line in r.stdout.splitlines()]
    assert len(out) == len(batches)
    return out


def border_rows(b, i):
    """nb = nb0 + the separators of window i"""
    nb0 = M.arrow_border(b, i)
    return nb0 + M.arrow_nseg(int(b.counts[i, 0]) - nb0) - 1


def test_the_two_functions_are_build_arrow_aux_window_by_window(driver, tmp_path):
    rng = np.random.default_rng(131)
    n0s = [2, 23, 24, 47, 48, 71, 72, 95, 96, 131]                                                       # every cut: one .. four segments
    batches = [W.arrow_batch(rng, [(n0, int(rng.integers(1, 13))) for n0 in n0s]),                      # ragged, poisoned beyond every count
               W.arrow_batch(rng, [(n0, nb0) for n0, nb0 in zip(n0s, (12, 1, 12, 1, 12, 1, 12, 1, 12, 1))]),
               W.arrow_batch(rng, [(n0, nb0) for n0, nb0 in zip(n0s, (1, 12, 1, 12, 1, 12, 1, 12, 1, 12))])]
    batches += [W.arrow_batch(rng, [(int(rng.integers(2, 140)), int(rng.integers(1, 13))) for _ in range(int(rng.integers(1, 6)))]) for _ in range(6)]
    for b, o in zip(batches, run(driver, tmp_path, batches)):
        assert (o["verdict"], o["first"], o["code"], o["batch"]) == (1, -1, OK, 0), o
        assert o["nb_max"] == max(border_rows(b, i) for i in range(b.n))
        assert 1 <= o["jmax"] <= 64 and 1 <= o["jpmax"] <= 16 and o["list_cap"] >= 1


def test_every_refusal(driver, tmp_path):
    gap = subprocess.run([driver, "--info"], capture_output=True, text=True)
    assert gap.returncode == 0 and gap.stderr == "" and gap.stdout.split() == ["gap", str(CHAIN_GAP)]   # (no admitted window reaches it: asked directly)

    def window(n0, nb0, nv_max=None, n_anchors=300, extra=0, np_max=20):
        b = Batch(1, nv_max or n0 + nb0 + 1, n0 + nb0 + 70 + extra, np_max, 1, nv_max or n0 + nb0 + 1, n_anchors=n_anchors)
        for k in range(n0 + nb0):
            b.add_pose(0)
        for k in range(1, n0):
            b.add_range(0, k - 1, k)
        for a in range(nb0):
            b.add_range(0, 0, n0 + a)
        return b
    cases = [(window(5, 1), OK, 0), (window(5, 12), OK, 0), (window(2, 3), OK, 0)]
    cases += [(window(5, 0), BORDER, 0), (window(5, 13), BORDER, 0), (window(1, 1), BORDER, 0)]        # a chain; nb0 = 13; nv - nb0 < 2
    b = window(5, 2); b.add_range(0, 2, 1); cases.append((b, PAIR_TWICE, 0))
    b = window(5, 2); b.add_range(0, 5, 6); b.add_range(0, 6, 5); cases.append((b, OK, 0))             # (on a border pair it is fine)
    b = window(5, 2); b.add_range(0, 3, -256); cases.append((b, OK, 0))                                # anchor index 255
    b = window(5, 2); b.add_range(0, 3, -257); cases.append((b, ANCHOR_CODE, 0))
    b = window(5, 2); b.add_range(0, 6, 6); cases.append((b, SELF_RANGE, 0))                           # (check_instances refuses the row before)
    for count, batch in ((63, 0), (64, BATCH_SIZES)):                                                  # row 1 owns its link to row 0: 64 / 65 records
        b = window(5, 2)
        for _ in range(count):
            b.add_range(0, 1, -1)
        cases.append((b, OK, batch))
    for count, batch in ((16, 0), (17, BATCH_SIZES)):
        b = window(5, 2)
        for _ in range(count):
            b.add_prior(0, 6)
        cases.append((b, OK, batch))
    small, large = 528, 529                                                                           # the LDS limit at 15 border rows
    assert M.arrow3_lds_bytes(small, 15) <= M.ARROW_LDS_LIMIT < M.arrow3_lds_bytes(large, 15)
    cases += [(window(96, 12, nv_max=small), OK, 0), (window(96, 12, nv_max=large), OK, BATCH_LDS), (window(96, 11, nv_max=large), OK, 0)]
    # a refused window behind taken ones: its index is reported, and the batch is refused
    two = W.arrow_batch(np.random.default_rng(5), [(30, 3), (6, 2), (50, 4)])
    e = int(two.counts[1, 1])
    two.r_idx[1, e] = two.r_idx[1, [k for k in range(e) if abs(int(two.r_idx[1, k, 0]) - int(two.r_idx[1, k, 1])) == 1 and max(two.r_idx[1, k]) < 6][0]]
    two.r_val[1, e] = (1.0, 1.0, 0.0, 0.0, 0.0)
    two.counts[1, 1] = e + 1
    out = run(driver, tmp_path, [c[0] for c in cases] + [two])
    for (b, code, batch), o in zip(cases, out):
        assert (o["verdict"], o["code"], o["batch"]) == (int(code == OK and batch == 0), code, batch), (o, code, batch)
        assert o["first"] == (-1 if code == OK else 0)
    assert (out[-1]["verdict"], out[-1]["first"], out[-1]["code"]) == (0, 1, PAIR_TWICE)
