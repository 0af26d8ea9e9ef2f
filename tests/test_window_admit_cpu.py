"""The per-window rule of loc_window_upload_dev (localization_amd/csrc/window_admit.h; DESIGN.md §2, "Upload from device arrays") without a GPU.
window_admit and window_structure_flags — what window_admit_kernel.hip restates lane-parallel — run window by window through the stand-alone
driver tests/host/window_admit_driver.cpp (g++, AddressSanitizer + UBSan; every window's tables at exactly the size its counts name), which
reduces them and holds the result to window_structure.cpp's batch passes on the same tables (check_instances, chain_scan(ordered),
translation_only with both values of its flag, max_anchor_referenced) and topology_from_flags to batch_topology for every combination of the
wave6 fit, the wave6_se3 fit and structured_pinfo (options "tree" and "arrow3" 0).  The driver exits with 1 on any difference.  Here the
driver's output is also held to tests/_window_structure_model.py and to the verdicts the batches were built for."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _window_structure_model as M
from _window_structure_model import Batch, I32_MAX, I32_MIN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "localization_amd", "csrc")
GENERAL, CHAIN, CHAIN3, WAVE6, WAVE6S = 0, 1, 2, 7, 8
CHAINBIT, SINGLE_L, SINGLE_R, SINGLE_S, ANY_S, TRANS, TRANS_SKIP = 1, 2, 4, 8, 16, 32, 64


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("window_admit_driver")
    cxx = shutil.which("g++")
    assert cxx is not None, "g++ is needed to build tests/host/window_admit_driver.cpp (the project's build() needs it as well)"
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    rocm = os.path.dirname(os.path.dirname(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")))
    src = [os.path.join(ROOT, "tests", "host", "window_admit_driver.cpp"), os.path.join(CSRC, "window_structure.cpp"), os.path.join(CSRC, "window_dispatch.cpp")]
    logs = []
    for extra in (["-static-libasan", "-static-libubsan"], []):   # (the runtimes as archives where the compiler has them)
        r = subprocess.run([cxx, "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), "-I", CSRC, "-pthread", *flags, *extra, *src,
                            "-o", str(d / "driver")], capture_output=True, text=True)
        logs.append(" ".join(extra) + ": " + r.stderr[-1500:])
        if r.returncode == 0:
            return str(d / "driver")
    raise AssertionError("\n".join(logs))


def run(driver, tmp_path, batches, name="in"):
    """every batch through the driver (no difference from window_structure.cpp / batch_topology, nothing on stderr); one dict per batch"""
    path = tmp_path / f"{name}.bin"
    with open(path, "wb") as f:
        for b in batches:
            b.write(f)
    r = subprocess.run([driver, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-3000:])
    out = []
    for line in r.stdout.splitlines():
        head, verdicts, codes = (part.split() for part in line.split("|"))
        first, code, and_bits, or_bits, anchor = (int(x) for x in head)
        out.append(dict(first=first, code=code, and_bits=and_bits, or_bits=or_bits, anchor=anchor, verdicts=[int(x) for x in verdicts], codes=[int(x) for x in codes]))
    assert len(out) == len(batches)
    for b, o in zip(batches, out):                       # the numpy model, window by window and for the batch
        want = [M.first_failed_check(b, i) for i in range(b.n)]
        assert o["codes"] == want, (o["codes"], want)
        bad = [i for i, c in enumerate(want) if c]
        assert (o["first"], o["code"]) == ((bad[0], want[bad[0]]) if bad else (-1, 0))
        if not bad:
            chain, single, se3 = M.chain_scan(b, True)
            assert bool(o["and_bits"] & CHAINBIT) == chain
            if chain:
                assert bool(o["and_bits"] & SINGLE_L) == single
                assert (bool(o["or_bits"] & ANY_S) and bool(o["and_bits"] & SINGLE_R) and bool(o["and_bits"] & SINGLE_S)) == se3
            used = [int(-v) for i in range(b.n) for v in b.r_idx[i, :b.counts[i, 1], 1].tolist() if v < 0]
            assert o["anchor"] == max(used, default=0)
    return out


# ---- batches of every verdict ---------------------------------------------------------------------------------------------------

def chain_batch(rng, kind, n=6, nv_max=8, poison=True):
    """n windows of the chain family: "chain3" translation-only, "wave6" 6-DoF with single pairs, "wave6s" an EdgeSE3 per pair, "chain" a
    second range on one pair, "general" a loop edge.  Rows beyond every count hold garbage (Batch's poison)."""
    b = Batch(n, nv_max, 3 * nv_max, nv_max, nv_max, nv_max - 1, n_anchors=5)
    for i in range(n):
        nv = 0 if (kind != "general" and i == n - 2) else int(rng.integers(3, nv_max + 1))     # an empty window in every chain batch
        rot = None
        if kind != "chain3":
            a = rng.normal()
            rot = [[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]
        for k in range(nv):
            b.add_pose(i, rng.normal(size=3), R=rot)
        for k in range(nv):
            if k:
                b.add_range(i, *((k - 1, k) if rng.random() < 0.5 else (k, k - 1)), lever=(0.0, 0.0, 0.0) if kind == "chain3" else (0.1, 0.0, 0.2))
                if kind == "chain" and k == 2 and i == 1:
                    b.add_range(i, k, -1 - int(rng.integers(5)))
                    b.add_range(i, k, k - 1)                               # the pair again, after an anchor row in between
            if rng.random() < 0.7:
                b.add_range(i, k, -1 - int(rng.integers(5)))
            if rng.random() < 0.6:
                b.add_prior(i, k, rng.normal(size=3), info=(1.0, 2.0, 3.0, 0.0, 0.0, 0.0) if kind == "chain3" else (1.0, 2.0, 3.0, 4.0, 5.0, 6.0), R=rot)
            if k and kind == "wave6s":
                b.add_se3(i, *((k - 1, k) if rng.random() < 0.5 else (k, k - 1)))
        if kind == "general" and i == n - 1 and nv >= 3:
            b.add_range(i, 0, nv - 1)                                      # a loop edge
    return b


WANT = {"chain3": [CHAIN3] * 8, "wave6": [CHAIN, WAVE6, CHAIN, WAVE6] * 2, "wave6s": [CHAIN, CHAIN, WAVE6S, WAVE6S] * 2, "chain": [CHAIN] * 8, "general": [GENERAL] * 8}


@pytest.mark.parametrize("kind", list(WANT))
def test_random_valid_batches_of_each_verdict(driver, tmp_path, kind):
    rng = np.random.default_rng(list(WANT).index(kind) + 40)
    batches = [chain_batch(rng, kind) for _ in range(5)]
    for o in run(driver, tmp_path, batches, kind):
        assert o["first"] == -1 and o["verdicts"] == WANT[kind], (kind, o)
        assert bool(o["and_bits"] & TRANS) == (kind == "chain3")


def test_flavours_of_the_chain_scan(driver, tmp_path):
    """tests/test_window_structure_cpu.py's single windows: orderings, second rows, skipped poses"""
    import test_window_structure_cpu as S
    rng = np.random.default_rng(12)
    batches = [S.chain_window(rng, flavour) for flavour in S.FLAVOURS for _ in range(10)]
    batches += [S.small_windows(5 + seed, seed=300 + seed, chains=bool(seed % 2)) for seed in range(8)]
    run(driver, tmp_path, batches)


def plant(base, i, code):
    """one entry of window i of a valid batch changed so that check `code` fails there, and no earlier one"""
    b = base.copy("counts", "r_idx", "p_idx", "s_idx")
    nv = int(base.counts[i, 0])
    if code == 1:
        b.counts[i, i % 4] = base.caps[i % 4] + 1 if i % 2 else -1
    elif code == 2:
        b.r_idx[i, 0] = [(nv, 0), (0, nv), (-1, 1), (1, -1 - base.n_anchors), (1, 1)][i % 5]
    elif code == 3:
        b.r_idx[i, 0] = (0, 3) if i % 2 else (3, 0)
    elif code == 4:
        b.p_idx[i, 0] = nv if i % 2 else -1
    elif code == 5:
        b.s_idx[i, 0, :2] = [(nv, 0), (0, nv), (-1, 1), (1, -1), (2, 2)][i % 5]
    else:
        b.s_idx[i, 0, :2] = (0, 3) if i % 2 else (3, 0)
    return b


def refusal_base(rng, n=7):
    """valid windows of >= 4 poses with a range, a prior and an EdgeSE3 in row 0, bw_max = 2"""
    b = Batch(n, 6, 12, 4, 6, 2, n_anchors=3)
    for i in range(n):
        nv = int(rng.integers(4, 7))
        for k in range(nv):
            b.add_pose(i, rng.normal(size=3))
        for k in range(1, nv):
            b.add_range(i, k - 1, k)
            b.add_range(i, k, -1 - int(rng.integers(3)))
            b.add_se3(i, k, k - 1)
        b.add_prior(i, 0); b.add_prior(i, nv - 1)
    return b


@pytest.mark.parametrize("code", [1, 2, 3, 4, 5, 6])
def test_each_code_in_the_first_a_middle_and_the_last_window(driver, tmp_path, code):
    base = refusal_base(np.random.default_rng(code))
    where = (0, 3, base.n - 1)
    out = run(driver, tmp_path, [base] + [plant(base, i, code) for i in where] + [plant(plant(base, 5, code), 2, 7 - code)])
    assert out[0]["first"] == -1
    assert [(o["first"], o["code"]) for o in out[1:4]] == [(i, code) for i in where]
    assert (out[4]["first"], out[4]["code"]) == (2, 7 - code)           # two refused windows: the lower index is reported


def test_two_codes_in_one_window_the_first_in_check_order_wins(driver, tmp_path):
    base = refusal_base(np.random.default_rng(9))
    batches, want = [], []
    for first in range(1, 7):
        for second in range(first + 1, 7):
            b = plant(plant(base, 3, second), 3, first)
            if first == 1:
                b.counts[3] = base.counts[3]; b.counts[3, 3] = base.caps[3] + 1     # (the SE3 count: the rows of the other tables stay readable)
            if (first, second) in ((2, 3), (5, 6)):                     # the same row cannot fail both: the width in row 0, the index in row 1
                table = b.r_idx if first == 2 else b.s_idx
                table[3, 0, :2] = (0, 3); table[3, 1, :2] = (1, 1)
                want.append(second)
            else:
                want.append(first)
            batches.append(b)
    out = run(driver, tmp_path, batches)
    assert [(o["first"], o["code"]) for o in out] == [(3, c) for c in want]
    # the order inside one table: row 0's width comes before row 1's index, and row 0's index before its own width
    b = base.copy("r_idx"); b.r_idx[3, 0] = (5, 5)
    assert run(driver, tmp_path, [b])[0]["code"] == 2


def test_garbage_beyond_every_count_changes_nothing(driver, tmp_path):
    rng = np.random.default_rng(3)
    for kind in WANT:
        a = chain_batch(rng, kind)
        g = a.copy("poses", "r_idx", "p_idx", "s_idx", "r_val", "p_val", "s_val")
        for i in range(a.n):
            nv, nr, npr, ns = (int(x) for x in a.counts[i])
            g.poses[i, nv:] = 7.0; g.r_idx[i, nr:] = (0, 0); g.p_idx[i, npr:] = -5; g.s_idx[i, ns:] = (I32_MAX, I32_MIN, 1, 1)
            g.r_val[i, nr:] = 1.0; g.p_val[i, npr:] = 2.0; g.s_val[i, ns:] = np.inf
        oa, og = run(driver, tmp_path, [a, g], kind)
        assert oa == og and oa["verdicts"] == WANT[kind]


def test_negative_zero_in_a_rotation_and_in_a_lever_arm(driver, tmp_path):
    base = chain_batch(np.random.default_rng(5), "chain3")
    i = next(i for i in range(base.n) if base.counts[i, 2] > 0)
    lever = base.copy("r_val"); lever.r_val[i, 0, 3] = -0.0              # by value: still translation-only
    info = base.copy("p_val"); info.p_val[i, 0, 16] = -0.0
    rot = base.copy("poses"); rot.poses[i, 1, 1] = -0.0                  # by bits: not the identity
    prot = base.copy("p_val"); prot.p_val[i, 0, 3] = -0.0
    nan = base.copy("r_val"); nan.r_val[i, 0, 2] = np.nan
    diag = base.copy("p_val"); diag.p_val[i, 0, 15] = 1e-300             # rotation information: only the skipping verdict survives
    out = run(driver, tmp_path, [base, lever, info, rot, prot, nan, diag])
    both = TRANS | TRANS_SKIP
    assert [o["and_bits"] & both for o in out] == [both, both, both, 0, 0, 0, TRANS_SKIP]
    assert [o["verdicts"] == [CHAIN3] * 8 for o in out[:6]] == [True] * 3 + [False] * 3
    assert out[6]["verdicts"][:4] != [CHAIN3] * 4 and out[6]["verdicts"][4:] == [CHAIN3] * 4      # structured_pinfo reads the skipping flag
    big = base.copy(); big.n_anchors = 500001
    assert run(driver, tmp_path, [big])[0]["and_bits"] & both == 0


def test_windows_without_poses(driver, tmp_path):
    b = Batch(3, 4, 4, 2, 2, 3, n_anchors=1)
    out = run(driver, tmp_path, [b])[0]
    assert out["first"] == -1 and out["verdicts"] == [CHAIN3] * 8 and out["anchor"] == 0
    r = b.copy("counts"); r.counts[1, 1] = 1                             # a row of a window without poses names no pose
    r = r.copy("r_idx"); r.r_idx[1, 0] = (0, -1)
    assert (lambda o: (o["first"], o["code"]))(run(driver, tmp_path, [r])[0]) == (1, 2)
