"""Test helper: the checkers of the full-information priors (loc_window_set_prior_information) and of the marginal prior of a dropped pose
(loc_window_marginal_prior_host), on the CPU oracle's general graph and numpy alone.

oracle_window / hessian / covariance_ref are tests/_oracle_window.py and tests/_covariance_ref.py with WindowBatch.p_info honoured: a prior
enters the oracle with its full 6 x 6 matrix (Graph.add_prior_edge takes one).  marginal_ref is the numpy statement of DESIGN.md §2, "The
marginal prior of a dropped pose"; marginal_by_elimination is the dense elimination it is checked against
(tests/test_marginal_prior_cpu.py)."""
import numpy as np

from _covariance_ref import cauchy_rho1

REL_PIVOT = 1e-11   # cov_device.h: kCovRelPivot (the pivot rule's constant, and the eigenvalue cut of the marginal)
LOC_ERR_SINGULAR = -6
BASE = 1000


def prior_information(wb, i, e):
    """the 6 x 6 information matrix of prior e of window i: its p_info row, or diag(p_val[12..17])"""
    if getattr(wb, "p_info", None) is not None:
        return wb.p_info[i, e].reshape(6, 6).copy()
    return np.diag(wb.p_val[i, e, 12:18])


def graph(wb, i, anchors, poses=None):
    """(oracle graph of window i at `poses` (default wb.poses[i]), edges): edges[k] = (pose slots — None for a fixed endpoint —,
    information, robust, kind) in the order range, prior, SE3 = the oracle's edge index"""
    from oracle import oracle as O
    poses = wb.poses[i] if poses is None else poses
    nv, nr, np_, ns = (int(x) for x in wb.counts[i])
    G = O.Graph()
    for m, a in enumerate(np.asarray(anchors, dtype=float).reshape(-1, 3)):
        G.add_vertex(m, a, fixed=True)
    for k in range(nv):
        G.add_vertex(BASE + k, poses[k, 9:], poses[k, :9].reshape(3, 3))
    edges = []
    for e in range(nr):
        v0, v1 = int(wb.r_idx[i, e, 0]), int(wb.r_idx[i, e, 1])
        G.add_range_edge(BASE + v0, (-1 - v1) if v1 < 0 else BASE + v1, wb.r_val[i, e, 0], wb.r_val[i, e, 1], off0=wb.r_val[i, e, 2:5].copy())
        edges.append(((v0, v1 if v1 >= 0 else None), np.array([[wb.r_val[i, e, 1]]]), True, "range"))
    for e in range(np_):
        Ri = wb.p_val[i, e, :9].reshape(3, 3); ti = wb.p_val[i, e, 9:12]
        info = prior_information(wb, i, e)
        G.add_prior_edge(BASE + int(wb.p_idx[i, e]), -Ri.T @ ti, Ri.T, info)
        edges.append(((int(wb.p_idx[i, e]), None), info, False, "prior"))
    for e in range(ns):
        Ri = wb.s_val[i, e, :9].reshape(3, 3); ti = wb.s_val[i, e, 9:12]
        info = wb.s_val[i, e, 12:].reshape(6, 6)
        G.add_se3_edge(BASE + int(wb.s_idx[i, e, 0]), BASE + int(wb.s_idx[i, e, 1]), -Ri.T @ ti, Ri.T, info, bool(wb.s_idx[i, e, 2]))
        edges.append(((int(wb.s_idx[i, e, 0]), int(wb.s_idx[i, e, 1])), info, bool(wb.s_idx[i, e, 2]), "se3"))
    return G, edges


def oracle_window(wb, i, anchors, iterations=10, jac_mode=None):
    """tests/_oracle_window.oracle_solve_instance with p_info honoured: (poses [nv][12], chi2, og_stats)"""
    from oracle import oracle as O
    jac_mode = O.JAC_ANALYTIC if jac_mode is None else jac_mode
    G, _ = graph(wb, i, anchors)
    nv = int(wb.counts[i, 0])
    _, st = G.optimize(iterations, jac_mode)
    out = np.zeros((nv, 12))
    for k in range(nv):
        R, t = G.estimate(BASE + k)
        out[k, :9] = R.reshape(9); out[k, 9:] = t
    return out, G.chi2(), st


def hessian(wb, i, anchors, jac_mode, poses=None):
    """H = sum_e J_e^T (rho'_e Omega_e) J_e at `poses`: [6 nv][6 nv] (tests/_covariance_ref.hessian with p_info honoured)"""
    G, edges = graph(wb, i, anchors, poses)
    nv = int(wb.counts[i, 0])
    H = np.zeros((6 * nv, 6 * nv))
    for k, (vs, info, robust, _) in enumerate(edges):
        err, J0, J1 = G.linearize(k, jac_mode)
        w = cauchy_rho1(err @ info @ err) if robust else 1.0
        Js = (J0, J1)
        for a, va in enumerate(vs):
            for b, vb in enumerate(vs):
                if va is not None and vb is not None:
                    H[6 * va:6 * va + 6, 6 * vb:6 * vb + 6] += Js[a].T @ (w * info) @ Js[b]
    return H


def covariance_ref(wb, i, anchors, jac_mode, poses=None):
    """(cov [nv][6][6], mask [nv], H): tests/_covariance_ref.reference_covariance with p_info honoured"""
    H = hessian(wb, i, anchors, jac_mode, poses)
    nv = int(wb.counts[i, 0])
    keep = np.diag(H) != 0.0
    Sig = np.zeros_like(H)
    if keep.any():
        Sig[np.ix_(keep, keep)] = np.linalg.inv(H[np.ix_(keep, keep)])
    cov = np.stack([Sig[6 * v:6 * v + 6, 6 * v:6 * v + 6] for v in range(nv)])
    mask = np.array([sum(1 << k for k in range(6) if not keep[6 * v + k]) for v in range(nv)], dtype=np.int32)
    return cov, mask, H


# ---- the marginal prior of a dropped pose ---------------------------------------------------------------------------------------------------
def neighbour(wb, i, d):
    """the one pose that pose-to-pose ranges join to pose d of window i (-1: none); asserts that there is at most one"""
    m = -1
    for e in range(int(wb.counts[i, 1])):
        v0, v1 = int(wb.r_idx[i, e, 0]), int(wb.r_idx[i, e, 1])
        if v1 >= 0 and d in (v0, v1):
            o = v1 if v0 == d else v0
            assert m in (-1, o)
            m = o
    return m


def removed_quadratic(wb, i, anchors, jac_mode, d, poses=None):
    """(m, H [6][6], g [6]) of the factors with d as an endpoint, over z = (t_d, t_m), linearised at `poses` by the covariance definition:
    H = sum J^T (rho' Omega) J, g = sum J^T (rho' Omega) e, in edge order (ranges, then priors)"""
    G, edges = graph(wb, i, anchors, poses)
    m = neighbour(wb, i, d)
    H = np.zeros((6, 6)); g = np.zeros(6)
    for k, (vs, info, robust, kind) in enumerate(edges):
        if d not in vs:
            continue
        assert kind != "se3"
        err, J0, J1 = G.linearize(k, jac_mode)
        w = cauchy_rho1(err @ info @ err) if robust else 1.0
        J = np.zeros((len(err), 6))
        for side, v in enumerate(vs):
            if v is None:
                continue
            assert v in (d, m)
            J[:, (0 if v == d else 3):(3 if v == d else 6)] = (J0, J1)[side][:, :3]
        H += J.T @ (w * info) @ J
        g += J.T @ (w * info) @ err
    return m, H, g


def ldl_pivots(A):
    """the LDL^T pivots of A in the natural order, each relative to its diagonal entry of A (stops at the first that is not positive)"""
    M = A.copy(); d0 = np.diag(A).copy(); out = []
    for j in range(len(M)):
        out.append(M[j, j] / d0[j])
        if not M[j, j] > 0:
            break
        M[j + 1:, j + 1:] -= np.outer(M[j + 1:, j], M[j, j + 1:]) / M[j, j]
    return np.array(out)


def marginal_ref(wb, i, anchors, jac_mode, d, poses=None):
    """The numpy statement of DESIGN.md §2, "The marginal prior of a dropped pose", for pose d of window i.  Returns a dict: slot, prior
    [48], grad [6], shift [6], rank, status as loc_window_marginal_prior_host writes them, and what the tests judge the inputs and the
    errors by: H, g (removed_quadratic), Hdd (after the exclusion), pivots (ldl_pivots of Hdd), Lam, gamma, eig (ascending), term
    (|g_m| + |H_md H_dd^-1 g_d|, the scale of gamma's error), kappa (of Hdd)."""
    poses = wb.poses[i] if poses is None else poses
    m, H, g = removed_quadratic(wb, i, anchors, jac_mode, d, poses)
    out = {"slot": m, "prior": np.zeros(48), "grad": np.zeros(6), "shift": np.zeros(6), "rank": 0, "status": 0, "H": H, "g": g}
    out["prior"][[0, 4, 8]] = 1.0
    if m < 0:   # nothing to carry the marginal
        return out
    tm = poses[m, 9:12]
    out["prior"][9:12] = -tm   # X_m^-1 (identity rotations)
    Hdd, Hmd, Hmm, gd, gm = H[:3, :3].copy(), H[3:, :3].copy(), H[3:, 3:], g[:3].copy(), g[3:]
    ex = np.diag(Hdd) == 0.0   # excluded coordinates of d
    Hdd[ex, :] = 0.0; Hdd[:, ex] = 0.0; Hdd[ex, ex] = 1.0; Hmd[:, ex] = 0.0; gd[ex] = 0.0
    piv = ldl_pivots(Hdd)
    out.update(Hdd=Hdd, pivots=piv, kappa=np.linalg.cond(Hdd))
    if len(piv) < 3 or not (piv > REL_PIVOT).all() or not np.isfinite(piv).all():
        out["status"] = LOC_ERR_SINGULAR   # the removed factors do not determine d: the zero row = the plain drop
        return out
    Ai = np.linalg.inv(Hdd)
    Lam = Hmm - Hmd @ Ai @ Hmd.T
    Lam = 0.5 * (Lam + Lam.T)
    carried = Hmd @ Ai @ gd
    gamma = gm - carried
    lam, V = np.linalg.eigh(Lam)
    keep = (lam > REL_PIVOT * lam.max()) & (lam > 0)
    info3 = (V[:, keep] * lam[keep]) @ V[:, keep].T
    e0 = V[:, keep] @ ((V[:, keep].T @ gamma) / lam[keep])
    info = np.zeros((6, 6)); info[:3, :3] = 0.5 * (info3 + info3.T)
    out["prior"][9:12] = e0 - tm
    out["prior"][12:] = info.reshape(36)
    out["grad"][:3] = gamma; out["shift"][:3] = e0
    out.update(rank=int(keep.sum()), Lam=Lam, gamma=gamma, eig=lam, term=np.linalg.norm(gm) + np.linalg.norm(carried))
    return out


def marginal_by_elimination(H, g, ex=None):
    """The removed factors' quadratic q(dd, dm) = 1/2 z^T H z + g^T z with dd minimised out, by least squares instead of the Schur complement:
    dd*(dm) = argmin is affine in dm — its constant and its slope come from np.linalg.lstsq on H_dd —, and q(dd*(dm), dm) =
    1/2 dm^T Lam dm + gamma^T dm + const is read off by substitution.  Returns (Lam, gamma)."""
    Hdd, Hdm = H[:3, :3], H[:3, 3:]
    c0 = np.linalg.lstsq(Hdd, -g[:3], rcond=None)[0]          # dd* at dm = 0
    S = np.linalg.lstsq(Hdd, -Hdm, rcond=None)[0]             # d dd* / d dm
    T = np.vstack([S, np.eye(3)])                             # z = T dm + (c0, 0)
    z0 = np.concatenate([c0, np.zeros(3)])
    Lam = T.T @ H @ T
    gamma = T.T @ (H @ z0 + g)
    return 0.5 * (Lam + Lam.T), gamma


def prior_residual(prior_row, pose):
    """toVectorMQT(Z^-1 X)'s translation part for a translation-only pose (identity rotations): Z^-1.R t + Z^-1.t"""
    return prior_row[:9].reshape(3, 3) @ pose[9:12] + prior_row[9:12]
