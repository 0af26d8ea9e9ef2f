"""The publish rule of a window (localization_amd/csrc/pose_records.h; DESIGN.md §2, "Publish and path records of a resident batch") without a
GPU.  The header is what window_publish_kernel.hip and the node's front end evaluate, so it is held here to the statement written from the
reference's behaviour (tests/_publish_ref.py: Eigen's Quaternion(Matrix3), tf::poseEigenToMsg's flip, the gate of Localization::publish(),
the ring-to-window slot rule) — through the stand-alone driver tests/host/pose_records_driver.cpp, compiled with g++
-fsanitize=address,undefined -ffp-contract=off and run as a program.  Every array a call reads or writes has exactly its size.

Everything is compared BIT FOR BIT (NaNs included: byte strings, not values)."""
import os
import shutil
import subprocess

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import _publish_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "localization_amd", "csrc")
SEED = 20261020


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("pose_records_driver")
    cxx = shutil.which("g++")
    assert cxx is not None, "g++ is needed to build tests/host/pose_records_driver.cpp (the project's build() needs it as well)"
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-Wall"]
    src = [os.path.join(ROOT, "tests", "host", "pose_records_driver.cpp")]
    logs = []
    for extra in (["-static-libasan", "-static-libubsan"], []):   # (the runtimes as archives where the compiler has them)
        r = subprocess.run([cxx, "-std=c++17", "-I", CSRC, *flags, *extra, *src, "-o", str(d / "driver")], capture_output=True, text=True)
        logs.append(" ".join(extra) + ": " + r.stderr[-1500:])
        if r.returncode == 0:
            return str(d / "driver")
    raise AssertionError("\n".join(logs))


def _run(driver, *args):
    r = subprocess.run([driver, *[str(a) for a in args]], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])


def _records(driver, tmp_path, poses, name):
    """the driver's records of poses [n][12], held bit for bit to the statement; returns them"""
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 12)
    src, dst = tmp_path / f"{name}.in", tmp_path / f"{name}.out"
    with open(src, "wb") as f:
        np.array([len(poses)], dtype=np.int32).tofile(f)
        poses.tofile(f)
    _run(driver, "records", src, dst)
    got = np.fromfile(dst, dtype=np.float64).reshape(-1, 7)
    assert len(got) == len(poses)
    for k, p in enumerate(poses):
        want = R.pose_record(p)
        assert got[k].tobytes() == want.tobytes(), (name, k, p.tolist(), got[k].tolist(), want.tolist())
    return got


def _pose(rot, t=(0.25, -1.5, 2.0)):
    m = rot.as_matrix() if isinstance(rot, Rotation) else np.asarray(rot, dtype=float)
    return np.concatenate([m.reshape(9), np.asarray(t, dtype=float)])


def _turn(axis, angle):
    a = np.asarray(axis, dtype=float)
    return Rotation.from_rotvec(a / np.linalg.norm(a) * angle)


def test_each_branch_and_its_flip(driver, tmp_path):
    """trace > 0, and each of the three largest-diagonal branches at 170 degrees; in those three a negative axis component gives w < 0 before
    the flip.  (The trace branch has w = 0.5 sqrt(trace + 1) > 0: it cannot flip.)"""
    poses, want = [_pose(_turn((1, 2, 3), 0.7))], [(0, False)]
    for i in range(3):
        for sign in (1.0, -1.0):
            # w = (m[k, j] - m[j, k]) t = 2 a_i sin(angle) t: its sign is the sign of the axis component
            axis = np.full(3, 0.1); axis[i] = sign
            poses.append(_pose(_turn(axis, np.deg2rad(170.0))))
            want.append((1 + i, sign < 0))
    for p, (br, fl) in zip(poses, want):
        assert R.branch(p[:9]) == br and R.quaternion_flipped(p[:9])[1] == fl, (p, br, fl)
    got = _records(driver, tmp_path, poses, "branches")
    assert (got[:, 6] >= 0).all()
    for p, g in zip(poses, got):   # the records are rotations: the quaternion turns back into the matrix
        assert np.allclose(Rotation.from_quat(g[3:]).as_matrix().reshape(9), p[:9], atol=1e-12)


def test_ties_zero_trace_half_turns_identity(driver, tmp_path):
    s = np.sqrt(0.5)
    cases = {
        # half turns about a face diagonal: 2 a a^T - 1 has two equal diagonal entries above the third
        "R00 == R11": (np.array([[0, 1, 0], [1, 0, 0], [0, 0, -1.0]]), 1),
        "R11 == R22": (np.array([[-1, 0, 0], [0, 0, 1], [0, 1, 0.0]]), 2),
        "R00 == R22": (np.array([[0, 0, 1], [0, -1, 0], [1, 0, 0.0]]), 1),
        # all three equal with trace <= 0: the half turn about (1, 1, 1) / sqrt 3 (diagonal 2/3 - 1 three times) ...
        "all equal, trace -1": (2.0 * np.full((3, 3), 1.0 / 3.0) - np.eye(3), 1),
        # ... and the 120 degree turns about it: permutation matrices, trace EXACTLY 0
        "trace 0": (np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0.0]]), 1),
        "trace 0, the other way": (np.array([[0, 1, 0], [0, 0, 1], [1, 0, 0.0]]), 1),
        "half turn x": (np.diag([1.0, -1, -1]), 1), "half turn y": (np.diag([-1.0, 1, -1]), 2), "half turn z": (np.diag([-1.0, -1, 1]), 3),
        "identity": (np.eye(3), 0),
        # the same ties from scipy's matrices (entries off by an ulp are fine: whichever way they fall, the statement decides)
        "scipy (1,1,0)": (_turn((s, s, 0), np.pi).as_matrix(), None), "scipy (0,1,1)": (_turn((0, s, s), np.pi).as_matrix(), None),
    }
    for name, (m, br) in cases.items():
        d = np.diag(m)
        if name.startswith("R") or name.startswith("all"):
            i, j = {"R00 == R11": (0, 1), "R11 == R22": (1, 2), "R00 == R22": (0, 2), "all equal, trace -1": (0, 1)}[name]
            assert d[i] == d[j] and np.trace(m) <= 0, name
        if name.startswith("all"):
            assert d[0] == d[1] == d[2]
        if name.startswith("trace 0"):
            assert m[0, 0] + m[1, 1] + m[2, 2] == 0.0
        assert br is None or R.branch(m.reshape(9)) == br, (name, R.branch(m.reshape(9)))
    got = _records(driver, tmp_path, [_pose(m) for m, _ in cases.values()], "ties")
    ident = got[list(cases).index("identity")]
    assert ident.tolist() == [0.25, -1.5, 2.0, 0.0, 0.0, 0.0, 1.0]
    q = got[list(cases).index("trace 0")][3:]
    assert np.allclose(q, [0.5, 0.5, 0.5, 0.5], atol=1e-15)   # 120 degrees about (1, 1, 1) / sqrt 3


def test_nan_entries_give_the_same_bits(driver, tmp_path):
    """a NaN in the rotation: off the diagonal in the trace branch and in a diagonal branch, and on the diagonal (every comparison false)"""
    poses = []
    for base, at in ((_turn((1, 2, 3), 0.7), 1), (_turn((1, 0.1, 0.1), 3.0), 5), (_turn((1, 2, 3), 0.7), 0), (_turn((0.1, 1, 0.1), 3.0), 4),
                     (_turn((0.1, 0.1, 1), 3.0), 8)):
        p = _pose(base); p[at] = np.nan
        poses.append(p)
    got = _records(driver, tmp_path, poses, "nan")
    assert np.isnan(got[:, 3:]).any(axis=1).all() and not np.isnan(got[:, :3]).any()


def test_random_rotations_up_to_pi(driver, tmp_path):
    rng = np.random.default_rng(SEED)
    axes = rng.normal(size=(1000, 3))
    angles = rng.uniform(0.0, np.pi, 1000); angles[:8] = np.pi
    poses = [_pose(_turn(a, th), rng.uniform(-5, 5, 3)) for a, th in zip(axes, angles)]
    seen = {(R.branch(p[:9]), R.quaternion_flipped(p[:9])[1]) for p in poses}
    assert {b for b, _ in seen} == {0, 1, 2, 3}, seen
    got = _records(driver, tmp_path, poses, "random")
    assert np.allclose(np.linalg.norm(got[:, 3:], axis=1), 1.0, atol=1e-12)


def test_publish_gate(driver, tmp_path):
    nan, inf = np.nan, np.inf
    thr = 1000.0
    pairs = [(999.5, thr, 1), (thr, thr, 0), (np.nextafter(thr, inf), thr, 0), (np.nextafter(thr, -inf), thr, 1),
             (nan, thr, 0), (nan, inf, 0), (12.5, inf, 1), (inf, inf, 0), (0.0, 0.0, 0), (-0.0, 0.0, 0), (1e300, np.nextafter(1e300, inf), 1)]
    src, dst = tmp_path / "gate.in", tmp_path / "gate.out"
    with open(src, "wb") as f:
        np.array([len(pairs)], dtype=np.int32).tofile(f)
        np.array([p[:2] for p in pairs], dtype=np.float64).tofile(f)
    _run(driver, "gate", src, dst)
    got = np.fromfile(dst, dtype=np.int32)
    assert got.tolist() == [p[2] for p in pairs]
    assert [int(R.gate(c, t)) for c, t, _ in pairs] == got.tolist()


def test_path_slot_for_every_small_ring(driver, tmp_path):
    dst = tmp_path / "slots.out"
    _run(driver, "slots", 6, dst)
    got = np.fromfile(dst, dtype=np.int32).tolist()
    want, at = [], 0
    for T in range(1, 7):
        for nv in range(T + 1):
            for i in range(T):
                want.append(R.path_slot(i, nv, T))
                s = got[at]; at += 1
                # the convention, independently of the formula: the newest pose is path index T - 1, the window holds the last nv indices
                assert (s >= 0) == (i >= T - nv) and s < max(nv, 1), (T, nv, i, s)
                if i == T - 1 and nv:
                    assert s == nv - 1
                if i == T - nv:
                    assert s == 0
    assert got == want


def test_windows_on_exactly_sized_arrays(driver, tmp_path):
    """every (nv, T) with T <= 6 — nv = 0 and nv = T + 1 (the caller's inconsistency) among them — published, gated and with a NaN chi2: the
    driver indexes heap arrays of exactly nv poses, 7-double records and T path rows under the sanitizers"""
    rng = np.random.default_rng(SEED + 1)
    cases = []
    for T in range(1, 7):
        for nv in range(T + 2):
            for chi2, thr in ((3.0, 4.0), (4.0, 4.0), (np.nan, np.inf)):
                x = np.stack([_pose(_turn(rng.normal(size=3), rng.uniform(0, np.pi)), rng.uniform(-3, 3, 3)) for _ in range(nv)]) if nv else np.zeros((0, 12))
                cases.append((nv, T, chi2, thr, x))
    src, dst = tmp_path / "windows.in", tmp_path / "windows.out"
    with open(src, "wb") as f:
        for nv, T, chi2, thr, x in cases:
            np.array([nv, T], dtype=np.int32).tofile(f)
            np.array([chi2, thr, R.POISON_D], dtype=np.float64).tofile(f)
            x.tofile(f)
    _run(driver, "windows", src, dst)
    raw = open(dst, "rb").read()
    at = 0
    for nv, T, chi2, thr, x in cases:
        counts = np.array([[nv, 0, 0, 0]], dtype=np.int32)
        poses = np.zeros((1, max(nv, 1), 12)); poses[0, :nv] = x
        result = np.zeros((1, 8)); result[0, 0] = chi2
        pd = lambda *shape: np.full(shape, R.POISON_D)
        flags, rt, opt, _, n = R.publish(counts, poses, result, thr, T, np.full(1, R.POISON_I, dtype=np.int32), pd(1, 7), pd(1, 7), pd(1))
        rows, present = R.path(counts, poses, T, 0, T, pd(1, T, 7), np.full((1, T), R.POISON_I, dtype=np.int32))
        want = flags.tobytes() + rt.tobytes() + opt.tobytes() + present.tobytes() + rows.tobytes()
        assert raw[at:at + len(want)] == want, (nv, T, chi2, thr)
        at += len(want)
        assert n == int(flags[0] & 1) and (nv <= T or (flags[0] == 0 and not present.any()))
    assert at == len(raw)
