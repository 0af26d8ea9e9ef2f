"""Test helper: the step that turns one raw message into a window's newest pose and its factors (loc_window_message_rows_dev; DESIGN.md §2,
"Rows from raw messages"), stated in Python / numpy float64 arithmetic from the reference's own text — Localization::addRangeEdge
(localization.cpp:297-376), Robot::new_vertex (robot.cpp:75-110), addImuEdge (:499-535), addLidarEdge (:462-496), addTwistEdge with twist2transform
and create_se3_edge_from_twist (:438-459, :560-605) — and not from localization_amd/csrc/message_rows.h.  Every operation is one IEEE double
operation in the reference's order (Python floats do not contract), so the library must reproduce it BIT FOR BIT; only sin and cos (math.sin /
math.cos here) come from another library than the device's: the twelve Z^-1 entries of a TWIST row with a non-zero angular rate are compared
under TWIST_BOUND.  MatrixXd::inverse() is stated as the node states it (Gauss-Jordan with partial pivoting, frontend.cpp's invert6 before
this change): the information of a TWIST row is compared bitwise as well.

It also holds the case table tests/test_message_rows_cpu.py and tests/test_gpu_message_rows.py share."""
import math

import numpy as np

RANGE, IMU, LIDAR, TWIST = 1, 2, 4, 8
NONE, APPENDED, REJECTED, INVALID, SINGULAR = 0, 1, 2, 3, 4
NR_NEW, NP_NEW, NS_NEW = 2, 2, 1
POISON_I, POISON_D = -77, -7.77e77

ANCH = np.array([[3, -3, 0.58], [3, 3, 1.97], [-3, 3, 0.54], [-3, -3, 1.76]], dtype=float)
ANTENNA = np.array([[0.1, 0.0, -0.05], [-0.2, 0.05, 0.0]])

# The twelve Z^-1 entries of a TWIST row whose angular rate is not zero: |device - this statement|.  Measured on an MI355X over four batches of
# 130 random TWIST windows (TWIST_SEEDS; angular rates up to a few rad/s, tests/test_gpu_message_rows.py prints the figure): 2.2e-16, one unit
# in the last place of an entry near 1 — the device's sin and cos differ from glibc's by a rounding and the products of three of them carry it
# into R.  Times 8 to cover other angles (never above 1e-13); rates ten times as large (half-angles up to 3 rad) were measured at 8.9e-16.
TWIST_SEEDS = (20261019, 20266020, 20266021, 20266022)
TWIST_MEASURED = 2.2204460492503131e-16
TWIST_BOUND = min(8 * TWIST_MEASURED, 1e-13)

# what tests/host/message_rows_driver.cpp writes per window
RECORD = np.dtype([("drop", "<i4"), ("nr", "<i4"), ("np", "<i4"), ("ns", "<i4"), ("verdict", "<i4"), ("r_idx", "<i4", (4,)), ("s_idx", "<i4", (4,)),
                   ("pad", "<i4"), ("pose", "<f8", (12,)), ("r_val", "<f8", (10,)), ("p_val", "<f8", (36,)), ("s_val", "<f8", (48,))])
FIELDS = ("drop", "nr", "np", "ns", "verdict", "r_idx", "s_idx", "pose", "r_val", "p_val", "s_val")


class Config:
    def __init__(self, T, vmax=5.0, outlier=1.0, antenna=ANTENNA):
        self.T, self.vmax, self.outlier = int(T), float(vmax), float(outlier)
        self.antenna = np.zeros((0, 3)) if antenna is None else np.ascontiguousarray(antenna, dtype=float).reshape(-1, 3)


# ---- the reference's arithmetic, operation by operation -------------------------------------------------------------------------------------------
def quat_to_R(w, x, y, z):
    """Eigen::Quaterniond(w, x, y, z).toRotationMatrix() (no normalisation: localization.cpp:509 relies on it), row-major"""
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    return [1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)]


def iso_inverse(R, t):
    """(R, t)^-1 = (R^T, -(R^T t)) with the sum taken left to right"""
    Ri = [R[j * 3 + i] for i in range(3) for j in range(3)]
    ti = [-((Ri[i * 3] * t[0] + Ri[i * 3 + 1] * t[1]) + Ri[i * 3 + 2] * t[2]) for i in range(3)]
    return Ri, ti


def invert6(A):
    """MatrixXd::inverse() of a 6 x 6 as the node forms it: Gauss-Jordan on [A | I] with partial pivoting; None if a pivot is 0 or not finite"""
    M = np.zeros((6, 12))
    M[:, :6] = np.asarray(A, dtype=float).reshape(6, 6)
    M[:, 6:] = np.eye(6)
    for c in range(6):
        p = c
        for r in range(c + 1, 6):
            if abs(M[r, c]) > abs(M[p, c]):
                p = r
        if M[p, c] == 0.0 or not math.isfinite(M[p, c]):
            return None
        if p != c:
            M[[c, p]] = M[[p, c]]
        M[c] = M[c] / M[c, c]
        for r in range(6):
            if r == c or M[r, c] == 0.0:
                continue
            M[r] = M[r] - M[r, c] * M[c]
    return M[:, 6:].reshape(36).copy()


def twist_transform(tw, dt):
    """twist2transform (localization.cpp:560-583): tf::Quaternion::setRPY(wx dt, wy dt, wz dt), tf::Matrix3x3::setRotation, translation v dt"""
    hr, hp, hy = tw[3] * dt * 0.5, tw[4] * dt * 0.5, tw[5] * dt * 0.5
    cy, sy, cp, sp, cr, sr = math.cos(hy), math.sin(hy), math.cos(hp), math.sin(hp), math.cos(hr), math.sin(hr)
    qx = sr * cp * cy - cr * sp * sy
    qy = cr * sp * cy + sr * cp * sy
    qz = cr * cp * sy - sr * sp * cy
    qw = cr * cp * cy + sr * sp * sy
    s = 2.0 / (((qx * qx + qy * qy) + qz * qz) + qw * qw)
    xs, ys, zs = qx * s, qy * s, qz * s
    wx, wy, wz, xx, xy, xz, yy, yz, zz = qw * xs, qw * ys, qw * zs, qx * xs, qx * ys, qx * zs, qy * ys, qy * zs, qz * zs
    R = [1.0 - (yy + zz), xy - wz, xz + wy, xy + wz, 1.0 - (xx + zz), yz - wx, xz - wy, yz + wx, 1.0 - (xx + yy)]
    return R, [tw[0] * dt, tw[1] * dt, tw[2] * dt]


def _information_ok(v):
    return math.isfinite(v) and v > 0.0


def _div(a, b):
    """IEEE a / b for Python floats (no ZeroDivisionError)"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def estimate(x, anchor):
    """distance_estimation of :306-307 between the vertex origins"""
    dx, dy, dz = (float(x[9 + k]) - float(anchor[k]) for k in range(3))
    return math.sqrt((dx * dx + dy * dy) + dz * dz)


def window_rows(cfg, mask, nv, x, anchors, msg):
    """One window.  nv: its count; x: its newest solved pose [12] (None when nv < 1); msg: dict(kind, dt, anchor, antenna, distance, distance_err
    — np.float32 —, imu [7], lidar_z, twist [42]); the entries a kind does not use are never read.  Returns dict(drop, pose [12], nr, np, ns,
    verdict, r_idx / r_val / p_val / s_idx / s_val: lists of the written rows)."""
    T = cfg.T
    drop = nv == T
    s = nv - int(drop)
    R = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0] if nv < 1 else [float(v) for v in x[:9]]
    t = [0.0, 0.0, 0.0] if nv < 1 else [float(v) for v in x[9:12]]
    out = dict(drop=int(drop), nr=-1, np=-1, ns=-1, r_idx=[], r_val=[], p_val=[], s_idx=[], s_val=[])
    kind = int(msg["kind"])
    dt = float(msg["dt"])
    legal = kind in (RANGE, RANGE | IMU, RANGE | LIDAR, RANGE | IMU | LIDAR, TWIST)

    def done(verdict):
        out["verdict"] = verdict
        out["pose"] = R + t
        return out

    if kind == 0:
        return done(NONE)
    if nv <= 0 or nv > T:
        return done(INVALID)
    if not legal or kind & ~mask:
        return done(INVALID)
    if kind & RANGE:
        a, ant = int(msg["anchor"]), int(msg["antenna"])
        if not (0 <= a < len(anchors)) or not (0 <= ant <= len(cfg.antenna)):
            return done(INVALID)
        d = float(np.float32(msg["distance"]))
        if cfg.outlier > 0 and drop and abs(estimate(R + t, anchors[a]) - d) > cfg.outlier:   # :306-313
            return done(REJECTED)
        e = float(np.float32(msg["distance_err"]))
        info0 = _div(1.0, e * e)                          # :318, create_range_edge's covariance.inverse()
        sd = cfg.vmax * dt / 3                            # :319
        info1 = _div(1.0, sd * sd)
        ci = [_div(1.0, float(msg["imu"][4 + k])) for k in range(3)] if kind & IMU else [1.0, 1.0, 1.0]   # :516-518
        if not _information_ok(info0) or (s > 0 and not _information_ok(info1)) or not all(_information_ok(v) for v in ci):
            return done(INVALID)
        off = [float(v) for v in cfg.antenna[ant - 1]] if ant > 0 else [0.0, 0.0, 0.0]   # :333-334
        out["r_idx"].append((s, -1 - a)); out["r_val"].append([d, info0] + off)            # :331-336
        if s > 0:
            out["r_idx"].append((s - 1, s)); out["r_val"].append([0.0, info1, 0.0, 0.0, 0.0])   # :338-340
        if kind & IMU:      # :505-525
            q = [float(v) for v in msg["imu"][:4]]
            R = quat_to_R(q[3], q[0], q[1], q[2])
            Ri, ti = iso_inverse(R, t)
            out["p_val"].append(Ri + ti + [0.0, 0.0, 0.0] + ci)
        if kind & LIDAR:    # :468-486
            t = [t[0], t[1], float(msg["lidar_z"])]
            Ri, ti = iso_inverse(R, t)
            out["p_val"].append(Ri + ti + [0.0, 0.0, 1 / 0.05, 0.0, 0.0, 0.0])
        out["nr"], out["np"], out["ns"] = len(out["r_idx"]), len(out["p_val"]), 0
        return done(APPENDED)
    # TWIST, :438-459 and :586-605
    if s == 0:
        return done(INVALID)
    tw = [float(v) for v in msg["twist"]]
    ZR, Zt = twist_transform(tw, dt)
    Ri, ti = iso_inverse(ZR, Zt)
    info = invert6([tw[6 + i] * dt * dt for i in range(36)])   # :579, :600
    if info is None:
        return done(SINGULAR)
    out["s_idx"].append((s - 1, s, 1, 0)); out["s_val"].append(Ri + ti + [float(v) for v in info])
    out["nr"], out["np"], out["ns"] = 0, 0, 1
    return done(APPENDED)


def batch_rows(cfg, mask, nv, x, anchors, msgs):
    """window_rows for a batch, into arrays poisoned where nothing is written: a structured array of RECORD (pad 0).  nv int [B]; x [B][12] the
    newest solved pose of every window (ignored where nv < 1); msgs: dict of arrays [B][...]"""
    B = len(nv)
    rec = np.zeros(B, dtype=RECORD)
    for f in ("r_idx", "s_idx"):
        rec[f] = POISON_I
    for f in ("r_val", "p_val", "s_val"):
        rec[f] = POISON_D
    for b in range(B):
        m = {k: (None if v is None else v[b]) for k, v in msgs.items()}
        o = window_rows(cfg, mask, int(nv[b]), None if nv[b] < 1 else x[b], anchors, m)
        r = rec[b]
        r["drop"], r["nr"], r["np"], r["ns"], r["verdict"] = o["drop"], o["nr"], o["np"], o["ns"], o["verdict"]
        r["pose"] = o["pose"]
        for e, (ix, val) in enumerate(zip(o["r_idx"], o["r_val"])):
            r["r_idx"][e * 2:e * 2 + 2] = ix; r["r_val"][e * 5:e * 5 + 5] = val
        for e, val in enumerate(o["p_val"]):
            r["p_val"][e * 18:e * 18 + 18] = val
        for ix, val in zip(o["s_idx"], o["s_val"]):
            r["s_idx"][:] = ix; r["s_val"][:] = val
    return rec


def assert_same_records(got, want, msgs, what=""):
    """every field of two RECORD arrays bitwise, except the Z^-1 of a TWIST row with a non-zero angular rate (TWIST_BOUND).  Returns the
    largest deviation seen there."""
    worst = 0.0
    assert len(got) == len(want), (what, len(got), len(want))
    for b in range(len(want)):
        for f in FIELDS:
            g, w = got[f][b], want[f][b]
            if f == "s_val" and want["ns"][b] == 1 and np.any(msgs["twist"][b][3:6] != 0.0):
                assert g[12:].tobytes() == w[12:].tobytes(), (what, b, "information", g[12:], w[12:])
                d = float(np.abs(g[:12] - w[:12]).max())
                worst = max(worst, d)
                assert d <= TWIST_BOUND, (what, b, "Z^-1 of a turning TWIST row", d, TWIST_BOUND)
            else:
                assert np.asarray(g).tobytes() == np.asarray(w).tobytes(), (what, b, f, g, w)
    return worst


# ---- messages ----------------------------------------------------------------------------------------------------------------------------------------
def empty_messages(B):
    return dict(kind=np.zeros(B, dtype=np.int32), dt=np.full(B, 1 / 32), anchor=np.zeros(B, dtype=np.int32), antenna=np.zeros(B, dtype=np.int32),
                distance=np.full(B, 3.0, dtype=np.float32), distance_err=np.full(B, 0.055, dtype=np.float32), imu=np.zeros((B, 7)),
                lidar_z=np.zeros(B), twist=np.zeros((B, 42)))


def masked(msgs, mask):
    """the arrays the mask requires (kind and dt always), None for the others"""
    need = dict(kind=True, dt=True, anchor=mask & RANGE, antenna=mask & RANGE, distance=mask & RANGE, distance_err=mask & RANGE, imu=mask & IMU,
                lidar_z=mask & LIDAR, twist=mask & TWIST)
    return {k: (v if need[k] else None) for k, v in msgs.items()}


def random_pose(rng):
    """a pose near the anchors' room with any attitude: R(9), t(3)"""
    q = rng.normal(size=4); q /= np.linalg.norm(q)
    return np.array(quat_to_R(q[3], q[0], q[1], q[2]) + [rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(0.5, 1.5)])


def fill_message(rng, msgs, b, kind, x, turning=True):
    """a plausible message of `kind` for a window whose newest pose is x"""
    msgs["kind"][b] = kind
    msgs["dt"][b] = rng.uniform(0.01, 0.1)
    a = int(rng.integers(len(ANCH)))
    msgs["anchor"][b], msgs["antenna"][b] = a, int(rng.integers(0, len(ANTENNA) + 1))
    msgs["distance"][b] = np.float32(np.linalg.norm(x[9:] - ANCH[a]) + rng.normal(0, 0.05))
    msgs["distance_err"][b] = np.float32(rng.uniform(0.03, 0.08))
    q = rng.normal(size=4); q /= np.linalg.norm(q)
    msgs["imu"][b] = np.concatenate([q, rng.uniform(1e-6, 1e-5, 3)])
    msgs["lidar_z"][b] = rng.uniform(0.5, 1.5)
    A = rng.normal(size=(6, 6))
    cov = (A @ A.T + 6 * np.eye(6)) * 1e-2
    msgs["twist"][b] = np.concatenate([rng.normal(0, 0.5, 3), rng.normal(0, 0.6, 3) * rng.choice([1.0, 10.0]) if turning else np.zeros(3), cov.reshape(36)])


LEGAL_KINDS = (RANGE, RANGE | IMU, RANGE | LIDAR, RANGE | IMU | LIDAR, TWIST)
RANDOM_SEED = 20261019


def random_batch(rng, B, T, kinds, nv_choices=None, none_share=0.05):
    """(nv [B], x [B][12], msgs): windows of 1 .. T poses with a random legal message each (kinds: what to draw from)"""
    nv = rng.choice(np.arange(1, T + 1) if nv_choices is None else nv_choices, B).astype(np.int32)
    x = np.stack([random_pose(rng) for _ in range(B)])
    msgs = empty_messages(B)
    for b in range(B):
        kind = 0 if rng.random() < none_share else int(rng.choice(kinds))
        fill_message(rng, msgs, b, kind, x[b])
        if rng.random() < 0.2:   # an outlier range: beyond most gates
            msgs["distance"][b] += np.float32(rng.choice([-1.0, 1.0]) * rng.uniform(0.4, 2.0))
    return nv, x, msgs


def neighbours32(v):
    """the float32 values just below and just above the double v (v itself left out when it is a float32)"""
    f = np.float32(v)
    lo = f if float(f) < v else np.nextafter(f, np.float32(-np.inf))
    hi = f if float(f) > v else np.nextafter(f, np.float32(np.inf))
    return lo, hi


def gate_cases(x, anchors, anchor, outlier):
    """float32 distances around both thresholds of the gate for newest pose x: [(distance, rejected)] by the statement's own rule, among them
    — where it exists — a distance with |est - d| == outlier exactly (accepted: the test is >)"""
    est = estimate(x, anchors[anchor])
    out = []
    for edge in (est - outlier, est + outlier):
        for d in neighbours32(edge) + (np.float32(edge),):
            out.append((np.float32(d), abs(est - float(d)) > outlier))
    return out


# ---- the invalid / singular causes: name -> (what to break in window b's message or count, the verdict) -------------------------------------------------
def _set(field, value):
    def f(msgs, nv, b):
        msgs[field][b] = value
    return f


def _imu_cov(k, value):
    def f(msgs, nv, b):
        msgs["imu"][b, 4 + k] = value
    return f


def _nv(value):
    def f(msgs, nv, b):
        nv[b] = value
    return f


def _twist_cov(fn):
    def f(msgs, nv, b):
        msgs["twist"][b, 6:] = fn(msgs["twist"][b, 6:].reshape(6, 6)).reshape(36)
    return f


def _rank5(c):
    c = c.copy(); c[5] = c[4]; c[:, 5] = c[:, 4]
    return c


# (cause, the kind the window's message has, the change, the verdict); T is the configuration's trajectory_length where a change needs it.
# TWIST with s == 0 needs T == 1 (s = nv - drop is 0 only for a one-pose window at its lag): the tests build it themselves.
def causes(T):
    return [
        ("none", RANGE, _set("kind", 0), NONE),
        ("nv_zero", RANGE, _nv(0), INVALID),
        ("nv_negative", RANGE, _nv(-3), INVALID),
        ("nv_beyond_T", RANGE, _nv(T + 1), INVALID),
        ("kind_imu_alone", RANGE | IMU, _set("kind", IMU), INVALID),
        ("kind_lidar_alone", RANGE | LIDAR, _set("kind", LIDAR), INVALID),
        ("kind_twist_and_range", RANGE, _set("kind", TWIST | RANGE), INVALID),
        ("kind_twist_and_imu", TWIST, _set("kind", TWIST | IMU), INVALID),
        ("kind_unknown_bit", RANGE, _set("kind", RANGE | 16), INVALID),
        ("kind_negative", RANGE, _set("kind", -1), INVALID),
        ("anchor_negative", RANGE, _set("anchor", -1), INVALID),
        ("anchor_beyond", RANGE, _set("anchor", len(ANCH)), INVALID),
        ("antenna_negative", RANGE, _set("antenna", -1), INVALID),
        ("antenna_beyond", RANGE, _set("antenna", len(ANTENNA) + 1), INVALID),
        ("err_zero", RANGE, _set("distance_err", np.float32(0.0)), INVALID),
        ("err_nan", RANGE, _set("distance_err", np.float32(np.nan)), INVALID),
        ("err_inf", RANGE, _set("distance_err", np.float32(np.inf)), INVALID),
        ("dt_zero", RANGE, _set("dt", 0.0), INVALID),
        ("dt_nan", RANGE, _set("dt", np.nan), INVALID),
        ("imu_cov0_zero", RANGE | IMU, _imu_cov(0, 0.0), INVALID),
        ("imu_cov4_negative", RANGE | IMU, _imu_cov(1, -1e-6), INVALID),
        ("imu_cov8_nan", RANGE | IMU | LIDAR, _imu_cov(2, np.nan), INVALID),
        ("twist_cov_zero", TWIST, _twist_cov(lambda c: c * 0.0), SINGULAR),
        ("twist_cov_rank5", TWIST, _twist_cov(_rank5), SINGULAR),
        ("twist_dt_zero", TWIST, _set("dt", 0.0), SINGULAR),
        ("twist_cov_nan", TWIST, _twist_cov(lambda c: c * np.nan), SINGULAR),
    ]
