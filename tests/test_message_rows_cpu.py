"""The rule that turns one raw message into a window's newest pose and its factors (localization_amd/csrc/message_rows.h; DESIGN.md §2, "Rows
from raw messages") without a GPU.  The header is what window_message_kernel.hip evaluates, so it is held here, window by window, to the
statement written from the reference (tests/_message_rows_ref.py) — through the stand-alone driver tests/host/message_rows_driver.cpp, compiled
with g++ -fsanitize=address,undefined -ffp-contract=off and run as a program.  Every array a window's call may read is handed over at exactly
its size, the outputs are poisoned first.

Everything is compared BIT FOR BIT, except the twelve Z^-1 entries of a TWIST row with a non-zero angular rate (sin and cos: TWIST_BOUND of the
helper; on the host both sides call glibc, so the deviation printed here is 0).  The last test feeds one window's messages through the node's
own front end (frontend.cpp compiled into the driver, every publish flag off: no solve, no GPU) and compares what each message added to the
graph with the same rows: the move of quat_to_R, iso_inverse, invert6 and the twist transform into the header changed no bit."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _message_rows_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "localization_amd", "csrc")
ALL = M.RANGE | M.IMU | M.LIDAR | M.TWIST


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("message_rows_driver")
    cxx = shutil.which("g++")
    assert cxx is not None, "g++ is needed to build tests/host/message_rows_driver.cpp (the project's build() needs it as well)"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")   # frontend.cpp includes capi_host.h, which includes the HIP runtime's header (no HIP call is made)
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-w", "-D__HIP_PLATFORM_AMD__", "-I",
             os.path.join(rocm, "include")]
    src = [os.path.join(ROOT, "tests", "host", "message_rows_driver.cpp")]
    logs = []
    for extra in (["-static-libasan", "-static-libubsan"], []):   # (the runtimes as archives where the compiler has them)
        r = subprocess.run([cxx, "-std=c++17", "-I", CSRC, *flags, *extra, *src, "-o", str(d / "driver")], capture_output=True, text=True)
        logs.append(" ".join(extra) + ": " + r.stderr[-1500:])
        if r.returncode == 0:
            return str(d / "driver")
    raise AssertionError("\n".join(logs))


def _write_batch(f, cfg, mask, nv, x, msgs):
    B = len(nv)
    np.array([cfg.T, len(cfg.antenna), len(M.ANCH), mask, B, 0], dtype=np.int32).tofile(f)
    np.array([cfg.vmax, cfg.outlier], dtype=np.float64).tofile(f)
    cfg.antenna.astype(np.float64).tofile(f)
    M.ANCH.astype(np.float64).tofile(f)
    for b in range(B):
        np.array([nv[b], msgs["kind"][b], msgs["anchor"][b], msgs["antenna"][b]], dtype=np.int32).tofile(f)
        np.array([msgs["distance"][b], msgs["distance_err"][b]], dtype=np.float32).tofile(f)
        np.array([msgs["dt"][b], msgs["lidar_z"][b]], dtype=np.float64).tofile(f)
        if nv[b] >= 1:
            np.asarray(x[b], dtype=np.float64).tofile(f)
        if mask & M.IMU:
            np.asarray(msgs["imu"][b], dtype=np.float64).tofile(f)
        if mask & M.TWIST:
            np.asarray(msgs["twist"][b], dtype=np.float64).tofile(f)


def _check(driver, tmp_path, batches, name):
    """batches: [(cfg, mask, nv, x, msgs)]; the driver's records against the statement; returns (records, the largest TWIST deviation)"""
    src, dst = tmp_path / f"{name}.in", tmp_path / f"{name}.out"
    with open(src, "wb") as f:
        for bt in batches:
            _write_batch(f, *bt)
    r = subprocess.run([driver, "rows", str(src), str(dst)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    got = np.fromfile(dst, dtype=M.RECORD)
    worst, at, out = 0.0, 0, []
    for cfg, mask, nv, x, msgs in batches:
        want = M.batch_rows(cfg, mask, nv, x, M.ANCH, M.masked(msgs, mask))
        g = got[at:at + len(nv)]
        worst = max(worst, M.assert_same_records(g, want, msgs, name))
        out.append(g)
        at += len(nv)
    assert at == len(got)
    return np.concatenate(out), worst


def test_every_kind_at_every_count(driver, tmp_path):
    """every legal kind, nv from 1 to T (s == 0 among them: T = 1, and nv = 1 of a longer window), antenna 0 and > 0, every mask that admits the kind"""
    rng = np.random.default_rng(M.RANDOM_SEED + 1)
    batches = []
    for T in (1, 2, 4):
        cfg = M.Config(T)
        for kind in M.LEGAL_KINDS:
            for mask in (kind, ALL):
                nvs = [n for n in range(1, T + 1) for _ in range(3)]
                nv = np.array(nvs, dtype=np.int32)
                x = np.stack([M.random_pose(rng) for _ in nvs])
                msgs = M.empty_messages(len(nvs))
                for b in range(len(nvs)):
                    M.fill_message(rng, msgs, b, kind, x[b])
                    msgs["antenna"][b] = b % 3   # 0, 1, 2
                    # (inside the gate: the decisions have a test of their own)
                    msgs["distance"][b] = np.float32(M.estimate(x[b], M.ANCH[msgs["anchor"][b]]) + 0.1)
                batches.append((cfg, mask, nv, x, msgs))
    got, _ = _check(driver, tmp_path, batches, "kinds")
    twist_first = (got["verdict"] == M.INVALID)
    assert (got["verdict"][~twist_first] == M.APPENDED).all()
    assert twist_first.sum() > 0 and (got["ns"][got["verdict"] == M.APPENDED].max() == 1)   # (TWIST with s == 0 is INVALID, every other window appended)
    assert set(got["nr"][got["verdict"] == M.APPENDED]) == {0, 1, 2} and set(got["np"][got["verdict"] == M.APPENDED]) == {0, 1, 2}


def test_every_invalid_and_singular_cause(driver, tmp_path):
    rng = np.random.default_rng(M.RANDOM_SEED + 2)
    T = 4
    cfg = M.Config(T)
    cs = M.causes(T)
    B = 2 * len(cs)
    nv = np.full(B, 3, dtype=np.int32)
    x = np.stack([M.random_pose(rng) for _ in range(B)])
    msgs = M.empty_messages(B)
    want = []
    for i, (name, kind, change, verdict) in enumerate(cs):
        for b in (2 * i, 2 * i + 1):   # the cause, and the same message without it
            M.fill_message(rng, msgs, b, kind, x[b])
            msgs["distance"][b] = np.float32(M.estimate(x[b], M.ANCH[msgs["anchor"][b]]) - 0.2)
        change(msgs, nv, 2 * i)
        want += [verdict, M.APPENDED]
    got, _ = _check(driver, tmp_path, [(cfg, ALL, nv, x, msgs)], "causes")
    assert got["verdict"].tolist() == want, [(c[0], g) for c, g in zip(cs, got["verdict"][::2])]
    bad = got["verdict"] != M.APPENDED
    assert (got["nr"][bad] == -1).all() and (got["np"][bad] == -1).all() and (got["ns"][bad] == -1).all()
    # a bit outside kinds_mask: every kind under every mask that lacks one of its bits
    batches = []
    for kind in M.LEGAL_KINDS:
        for mask in range(16):
            if kind & ~mask:
                m1 = M.empty_messages(1)
                M.fill_message(rng, m1, 0, kind, x[0])
                batches.append((cfg, mask, nv[1:2], x[:1], m1))
    got, _ = _check(driver, tmp_path, batches, "mask")
    assert (got["verdict"] == M.INVALID).all()


def test_gate_on_both_sides_of_the_threshold(driver, tmp_path):
    rng = np.random.default_rng(M.RANDOM_SEED + 3)
    T = 3
    batches, want = [], []
    for trial in range(12):
        x = M.random_pose(rng)
        a = int(rng.integers(len(M.ANCH)))
        outlier = float(rng.choice([1.0, 0.25, 0.7]))
        cases = M.gate_cases(x, M.ANCH, a, outlier)
        msgs = M.empty_messages(len(cases))
        for b, (d, rejected) in enumerate(cases):
            M.fill_message(rng, msgs, b, M.RANGE, x)
            msgs["anchor"][b], msgs["distance"][b] = a, d
        xs = np.repeat(x[None], len(cases), axis=0)
        # at its lag the window gates; the same messages to a shorter window and with the gate disabled (outlier 0 and < 0) are appended
        batches.append((M.Config(T, outlier=outlier), M.RANGE, np.full(len(cases), T, dtype=np.int32), xs, msgs))
        want += [M.REJECTED if r else M.APPENDED for _, r in cases]
        batches.append((M.Config(T, outlier=outlier), M.RANGE, np.full(len(cases), T - 1, dtype=np.int32), xs, msgs))
        batches.append((M.Config(T, outlier=0.0), M.RANGE, np.full(len(cases), T, dtype=np.int32), xs, msgs))
        batches.append((M.Config(T, outlier=-1.0), M.RANGE, np.full(len(cases), T, dtype=np.int32), xs, msgs))
        want += [M.APPENDED] * (3 * len(cases))
        # |est - d| == outlier exactly: accepted (the test is >), and rejected one unit in the last place below
        d = np.float32(M.estimate(x, M.ANCH[a]) + 0.5)
        exact = abs(M.estimate(x, M.ANCH[a]) - float(d))
        m1 = M.empty_messages(1)
        M.fill_message(rng, m1, 0, M.RANGE, x)
        m1["anchor"][0], m1["distance"][0] = a, d
        batches.append((M.Config(T, outlier=exact), M.RANGE, np.array([T], dtype=np.int32), x[None], m1))
        batches.append((M.Config(T, outlier=float(np.nextafter(exact, 0.0))), M.RANGE, np.array([T], dtype=np.int32), x[None], m1))
        want += [M.APPENDED, M.REJECTED]
    got, _ = _check(driver, tmp_path, batches, "gate")
    assert got["verdict"].tolist() == want
    assert M.REJECTED in want and want.count(M.REJECTED) >= 24


def test_random_windows(driver, tmp_path):
    rng = np.random.default_rng(M.RANDOM_SEED)
    batches = []
    for k in range(12):
        T = int(rng.integers(1, 7))
        cfg = M.Config(T, vmax=float(rng.uniform(1, 6)), outlier=float(rng.choice([1.0, 0.3, 0.0])), antenna=None if k % 4 == 3 else M.ANTENNA)
        nv, x, msgs = M.random_batch(rng, 40, T, M.LEGAL_KINDS)
        if cfg.antenna.shape[0] == 0:
            msgs["antenna"][:] = 0
        batches.append((cfg, ALL, nv, x, msgs))
    got, worst = _check(driver, tmp_path, batches, "random")
    assert len(got) >= 400
    seen = np.bincount(got["verdict"], minlength=5)
    print(f"random windows per verdict NONE .. SINGULAR: {seen.tolist()}; largest |Z^-1 deviation| of a turning TWIST row on the host: {worst:.3e} "
          f"(bound {M.TWIST_BOUND:.3e})")
    assert seen[M.APPENDED] > 200 and seen[M.NONE] > 0 and seen[M.REJECTED] > 0


def test_the_node_front_end_gives_the_same_bits(driver, tmp_path):
    """One window's messages through loc_node_add_range / _imu / _lidar / _twist (no publish flag: nothing is solved), against the rows of the
    same messages for a window that starts with the node's one pose.  The gate is kept out of it (the node counts messages, the batch poses)."""
    rng = np.random.default_rng(M.RANDOM_SEED + 4)
    T, n_msgs = 4, 10
    cfg = M.Config(T, vmax=5.0, outlier=1e9)
    start = np.array([0.3, -0.4, 1.1])
    x = np.concatenate([np.eye(3).reshape(9), start])
    kinds = [M.RANGE, M.RANGE | M.IMU, M.TWIST, M.RANGE | M.IMU | M.LIDAR, M.RANGE | M.LIDAR, M.TWIST, M.RANGE, M.RANGE | M.IMU, M.TWIST, M.RANGE | M.LIDAR]
    msgs = M.empty_messages(n_msgs)
    stamps, stamp = [], 100.0
    for k in range(n_msgs):
        M.fill_message(rng, msgs, k, kinds[k], x)
        stamp = stamp + float(msgs["dt"][k])
        stamps.append(stamp)
    src, dst = tmp_path / "node.in", tmp_path / "node.out"
    with open(src, "wb") as f:
        np.array([T, len(cfg.antenna), len(M.ANCH), n_msgs], dtype=np.int32).tofile(f)
        np.array([cfg.vmax, cfg.outlier], dtype=np.float64).tofile(f)
        cfg.antenna.tofile(f); M.ANCH.tofile(f); start.tofile(f)
        for k in range(n_msgs):
            np.array([msgs["kind"][k], msgs["anchor"][k], msgs["antenna"][k], 0], dtype=np.int32).tofile(f)
            np.array([msgs["distance"][k], msgs["distance_err"][k]], dtype=np.float32).tofile(f)
            np.array([stamps[k], msgs["lidar_z"][k]], dtype=np.float64).tofile(f)
            msgs["imu"][k].tofile(f); msgs["twist"][k].tofile(f)
    r = subprocess.run([driver, "node", str(src), str(dst)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    got = np.fromfile(dst, dtype=M.RECORD)
    assert len(got) == n_msgs
    nv, prev = 1, 0.0   # (the node's first vertex has stamp 0)
    for k in range(n_msgs):
        one = {f: v[k:k + 1].copy() for f, v in msgs.items()}
        one["dt"][0] = stamps[k] - prev   # the stamp difference as the node forms it
        prev = stamps[k]
        want = M.batch_rows(cfg, ALL, np.array([nv], dtype=np.int32), x[None], M.ANCH, one)[0]
        g = got[k]
        assert want["verdict"] == M.APPENDED and g["verdict"] == 0, (k, want["verdict"], g["verdict"])
        assert (g["nr"], g["np"], g["ns"]) == (want["nr"], want["np"], want["ns"]), k
        assert g["pose"].tobytes() == want["pose"].tobytes(), (k, "new vertex")
        if want["nr"]:
            assert g["r_idx"].tolist() == [1, want["r_idx"][1], 1, 1], (k, g["r_idx"])
            assert g["r_val"].tobytes() == want["r_val"].tobytes(), (k, g["r_val"], want["r_val"])
        n = 18 * int(want["np"])
        assert g["p_val"][:n].tobytes() == want["p_val"][:n].tobytes(), (k, "priors")
        if want["ns"]:
            assert g["s_idx"].tolist() == [1, 1, 1, 0], (k, g["s_idx"])
            assert g["s_val"].tobytes() == want["s_val"].tobytes(), (k, np.abs(g["s_val"] - want["s_val"]).max())
        x = want["pose"].copy()
        nv = min(nv + 1, T)
