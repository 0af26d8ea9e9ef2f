"""Test helper: the per-update marginal covariances of loc_snapshot_solve_*_cov / loc_fusion_solve_*_cov in numpy (definition in
DESIGN.md §2).  For every tag and epoch the update is rebuilt in the CPU oracle's general graph (the tag vertex, the fixed anchors, one range
edge per ACTIVE range, for fusion the IMU prior edge), linearised there at the GPU's returned estimate, weighted with og_cauchy_rho, and the
exactly-zero coordinates are dropped before np.linalg.inv.  Active ranges follow the gate rule on the prior the handle used: the previous
epoch's output (the initial state at k = 0), ungated before the warm-up epoch, invalid slots never active."""
import numpy as np

from _covariance_ref import cauchy_rho1

REL_PIVOT = 1e-11   # a pivot at most this fraction of its diagonal entry is singular


def quat_to_R(w, x, y, z):
    """Eigen's Quaternion::toRotationMatrix (no normalisation)"""
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, 1 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1 - (txx + tyy)]])


def active_ranges(anchors, dist_m, err_m, prior_t, k, gate, gate_from_epoch):
    """indices m of the ranges in H: valid (err > 0, both finite) and not rejected by the gate on the prior's origin"""
    out = []
    for m in range(len(anchors)):
        d, e = float(dist_m[m]), float(err_m[m])
        if not (e > 0 and np.isfinite(e) and np.isfinite(d)):
            continue
        if gate > 0 and k >= gate_from_epoch and abs(np.linalg.norm(prior_t - anchors[m]) - d) > gate:
            continue
        out.append(m)
    return out


def condition(H):
    """2-norm condition number of H's kept block (1 when nothing is kept)"""
    keep = np.diag(H) != 0.0
    return float(np.linalg.cond(H[np.ix_(keep, keep)])) if keep.any() else 1.0


def invert(H):
    """(Sigma, mask, ok): H^-1 with the exactly-zero-diagonal coordinates excluded (rows / columns 0, mask bits set); ok = False (and
    Sigma NaN) if a pivot of the LDL^T of the kept block is not finite, not positive or at most REL_PIVOT of its diagonal entry"""
    n = H.shape[0]
    keep = np.diag(H) != 0.0
    mask = sum(1 << i for i in range(n) if not keep[i])
    Sig = np.zeros_like(H)
    if not keep.any():
        return Sig, mask, True
    A = H[np.ix_(keep, keep)].copy()
    dg = np.diag(A).copy()
    ok = True
    for j in range(A.shape[0]):   # LDL^T pivots
        d = A[j, j]
        ok = ok and np.isfinite(d) and d > REL_PIVOT * dg[j]
        if not ok:
            break
        A[j + 1:, j + 1:] -= np.outer(A[j + 1:, j], A[j, j + 1:]) / d
    if not ok:
        return np.full_like(H, np.nan), mask, False
    Sig[np.ix_(keep, keep)] = np.linalg.inv(H[np.ix_(keep, keep)])
    return Sig, mask, True


def _range_terms(G, edges, jac_mode, ncols):
    H = np.zeros((ncols, ncols))
    for idx, (info, robust) in edges:
        err, J0, _ = G.linearize(idx, jac_mode)
        w = cauchy_rho1(float(err @ info @ err)) if robust else 1.0
        J = J0[:, :ncols]
        H += J.T @ (w * info) @ J
    return H


def snapshot_hessian(anchors, dist_m, err_m, pos, active, jac_mode):
    """3x3 translation block of H at `pos` over the ranges `active` (oracle 6-DoF vertex, rotation identity)"""
    from oracle import oracle as O
    G = O.Graph()
    G.add_vertex(1000, pos)
    for m, a in enumerate(anchors):
        G.add_vertex(m, a, fixed=True)
    edges = []
    for i, m in enumerate(active):
        info = 1.0 / float(err_m[m]) ** 2
        G.add_range_edge(1000, m, float(dist_m[m]), info)
        edges.append((i, (np.array([[info]]), True)))
    return _range_terms(G, edges, jac_mode, 3)


def snapshot_reference(anchors, dist, err, init, out_pos, jac_mode, gate=1.0, gate_from_epoch=1, use_gate=True, kappa=None):
    """dist / err [K][M][B], init [3][B], out_pos [K][3][B] (the GPU's).  Returns cov [K][B][3][3], mask [K][B], ok [K][B], n_active [K][B];
    kappa ([K][B] array): filled with the condition number of each H.  use_gate=False: every valid range (the check that the gate is
    honoured)."""
    anchors = np.asarray(anchors, dtype=float)
    K, M, B = dist.shape
    cov = np.zeros((K, B, 3, 3)); mask = np.zeros((K, B), np.int32); ok = np.zeros((K, B), bool); nact = np.zeros((K, B), np.int32)
    for b in range(B):
        prior = np.asarray(init[:, b], dtype=float)
        for k in range(K):
            act = active_ranges(anchors, dist[k, :, b], err[k, :, b], prior, k, gate if use_gate else 0.0, gate_from_epoch)
            p = np.asarray(out_pos[k, :, b], dtype=float)
            H = snapshot_hessian(anchors, dist[k, :, b], err[k, :, b], p, act, jac_mode)
            cov[k, b], mask[k, b], ok[k, b] = invert(H)
            if kappa is not None:
                kappa[k, b] = condition(H)
            nact[k, b] = len(act)
            prior = p
    return cov, mask, ok, nact


def fusion_hessian(anchors, offset, dist_m, err_m, imu_kb, t, R, prior_t, active, jac_mode):
    """6x6 H at (t, R) in VertexSE3's [dt (body), dq_xyz]: the IMU prior (measurement: the IMU rotation, translation prior_t; information
    diag(0, 0, 0, 1/c0, 1/c4, 1/c8), not robust) and the active ranges with the lever arm on the tag"""
    from oracle import oracle as O
    G = O.Graph()
    G.add_vertex(1000, t, R)
    info6 = np.diag([0.0, 0.0, 0.0, 1.0 / imu_kb[4], 1.0 / imu_kb[5], 1.0 / imu_kb[6]])
    G.add_prior_edge(1000, prior_t, quat_to_R(imu_kb[3], imu_kb[0], imu_kb[1], imu_kb[2]), info6)
    edges = [(0, (info6, False))]
    for m, a in enumerate(anchors):
        G.add_vertex(m, a, fixed=True)
    for i, m in enumerate(active):
        info = 1.0 / float(err_m[m]) ** 2
        G.add_range_edge(1000, m, float(dist_m[m]), info, off0=np.asarray(offset, dtype=float))
        edges.append((1 + i, (np.array([[info]]), True)))
    return _range_terms(G, edges, jac_mode, 6)


def fusion_reference(anchors, offset, dist, err, imu, init, out_pose, jac_mode, gate=3.0, gate_from_epoch=1, use_gate=True, kappa=None):
    """dist / err [K][M][B], imu [K][B][8], init [7][B], out_pose [K][7][B] (the GPU's: t, q xyzw).
    Returns cov [K][B][6][6], mask [K][B], ok [K][B], n_active [K][B]."""
    anchors = np.asarray(anchors, dtype=float)
    K, M, B = dist.shape
    cov = np.zeros((K, B, 6, 6)); mask = np.zeros((K, B), np.int32); ok = np.zeros((K, B), bool); nact = np.zeros((K, B), np.int32)
    for b in range(B):
        prior_t = np.asarray(init[:3, b], dtype=float)
        for k in range(K):
            act = active_ranges(anchors, dist[k, :, b], err[k, :, b], prior_t, k, gate if use_gate else 0.0, gate_from_epoch)
            t = np.asarray(out_pose[k, :3, b], dtype=float)
            qx, qy, qz, qw = out_pose[k, 3:7, b]
            H = fusion_hessian(anchors, offset, dist[k, :, b], err[k, :, b], imu[k, b], t, quat_to_R(qw, qx, qy, qz), prior_t, act, jac_mode)
            cov[k, b], mask[k, b], ok[k, b] = invert(H)
            if kappa is not None:
                kappa[k, b] = condition(H)
            nact[k, b] = len(act)
            prior_t = t
    return cov, mask, ok, nact
