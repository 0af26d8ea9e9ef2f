"""Test helper: what the reference reports of a window after a solve, stated in numpy from the reference's behaviour — Eigen's
Quaternion(Matrix3) (the trace branch, else the largest diagonal entry i found by two strict comparisons, j = (i + 1) % 3, k = (j + 1) % 3),
tf::poseEigenToMsg's flip to w >= 0, the gate `chi2 < minimum_optimize_error` of Localization::publish(), Robot::current_pose(),
path->poses[trajectory_length / 2], Robot::vertices2path() and the destructor's tail.  tests/test_pose_records_cpu.py holds
localization_amd/csrc/pose_records.h to it and tests/test_gpu_publish.py the device records, both bit for bit.

Every operation is one IEEE double operation (numpy scalars), in Eigen's order.  A window holds the newest nv of the ring's T poses: path
index i is slot i - (T - nv); the ring's older vertices were never measured and are absent."""
import numpy as np

POISON_D = np.frombuffer(np.array([0x7FF8DEADBEEF0123], dtype=np.uint64).tobytes(), dtype=np.float64)[0]   # (a quiet NaN with a payload: compare bytes)
POISON_I = -0x5A5A5A5B


def quaternion_flipped(R):
    """Eigen::Quaterniond(R) for the row-major 3 x 3 R (9 values), then the flip to w >= 0; ((x, y, z, w), whether the flip was taken)"""
    m = np.asarray(R, dtype=np.float64).reshape(3, 3)
    one, half = np.float64(1.0), np.float64(0.5)
    q = [None, None, None]
    with np.errstate(all="ignore"):
        t = m[0, 0] + m[1, 1] + m[2, 2]
        if t > 0:
            t = np.sqrt(t + one)
            w = half * t
            t = half / t
            q[0] = (m[2, 1] - m[1, 2]) * t
            q[1] = (m[0, 2] - m[2, 0]) * t
            q[2] = (m[1, 0] - m[0, 1]) * t
        else:
            i = 0
            if m[1, 1] > m[0, 0]:
                i = 1
            if m[2, 2] > m[i, i]:
                i = 2
            j = (i + 1) % 3
            k = (j + 1) % 3
            t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + one)
            q[i] = half * t
            t = half / t
            w = (m[k, j] - m[j, k]) * t
            q[j] = (m[j, i] + m[i, j]) * t
            q[k] = (m[k, i] + m[i, k]) * t
        flipped = bool(w < 0)
        if flipped:
            w, q = -w, [-v for v in q]
    return np.array([q[0], q[1], q[2], w], dtype=np.float64), flipped


def quaternion_xyzw(R):
    return quaternion_flipped(R)[0]


def branch(R):
    """which of Eigen's four branches R takes: 0 = trace > 0, 1 + i otherwise"""
    m = np.asarray(R, dtype=np.float64).reshape(3, 3)
    if m[0, 0] + m[1, 1] + m[2, 2] > 0:
        return 0
    i = 1 if m[1, 1] > m[0, 0] else 0
    return 1 + (2 if m[2, 2] > m[i, i] else i)


def pose_record(pose12):
    p = np.asarray(pose12, dtype=np.float64)
    return np.concatenate([p[9:12], quaternion_xyzw(p[:9])])


def gate(chi2, minimum_optimize_error):
    return bool(np.float64(chi2) < np.float64(minimum_optimize_error))


def path_slot(i, nv, T):
    return i - (T - nv)


def publish(counts, poses, result, minimum_optimize_error, T, flags, realtime, optimized, chi2):
    """the four per-window outputs of loc_window_publish_resident written into copies of the given (poisoned) arrays; returns them and n_published"""
    flags, realtime, optimized, chi2 = flags.copy(), realtime.copy(), optimized.copy(), chi2.copy()
    n = 0
    for b in range(len(counts)):
        nv = int(counts[b, 0])
        chi2[b] = result[b, 0]
        ok = 1 <= nv <= T
        so = path_slot(T // 2, nv, T)
        pub = ok and gate(result[b, 0], minimum_optimize_error)
        flags[b] = int(pub) | (2 if ok and so >= 0 else 0)
        if pub:
            n += 1
            realtime[b] = pose_record(poses[b, nv - 1])
            if so >= 0:
                optimized[b] = pose_record(poses[b, so])
    return flags, realtime, optimized, chi2, n


def path(counts, poses, T, first, count, rows, present):
    """loc_window_path_resident's outputs written into copies of the given (poisoned) arrays"""
    rows, present = rows.copy(), present.copy()
    for b in range(len(counts)):
        nv = int(counts[b, 0])
        for k in range(count):
            s = path_slot(first + k, nv, T)
            here = 1 <= nv <= T and s >= 0
            present[b, k] = int(here)
            if here:
                rows[b, k] = pose_record(poses[b, s])
    return rows, present


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
