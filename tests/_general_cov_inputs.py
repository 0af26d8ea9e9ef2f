"""Test helper: windows of general structure whose UNDAMPED H is regular, for the covariance tests of envelope_covariance_kernel.hip
(tests/test_gpu_general_covariance.py on the GPU, tests/test_general_covariance_cpu.py on the oracle and numpy alone), and the numpy model
of what that kernel does: the envelope of the caller's pose order, its block LDL^T and the selected inversion restricted to it.

Every window meant to pass is regular by the reference alone: a tag pose is ranged to all four anchors (as test_gpu_covariance._observable_batch
does), or sits on a full-information EdgeSE3 star whose key is ranged to all four anchors and whose other poses carry one range each; nothing
is left gauge-free."""
import numpy as np
from scipy.spatial.transform import Rotation

ANCH = np.array([[3, -3, 0.58], [3, 3, 1.97], [-3, 3, 0.54], [-3, -3, 1.76]], dtype=float)
LEVER = np.array([0.1, 0.0, -0.05])
IMU_INFO = np.array([0, 0, 0, 1, 1, 1.0]) / 4.592449e-06
SMOOTH_INFO = 1.0 / (5.0 * (1 / 32) / 3) ** 2


def _trajectory(rng, T, six_dof=True):
    tt = np.cumsum(rng.normal(0, 0.05, (T, 3)), axis=0) + np.array([rng.uniform(-1.5, 1.5), rng.uniform(-1.5, 1.5), 1.1])
    if six_dof:
        tR = Rotation.from_rotvec(np.cumsum(rng.normal(0, 0.03, (T, 3)), axis=0) + rng.normal(0, 0.3, 3))
        eR = (tR * Rotation.from_rotvec(rng.normal(0, 0.02, (T, 3)))).as_matrix()
    else:
        tR = Rotation.from_rotvec(np.zeros((T, 3)))
        eR = np.broadcast_to(np.eye(3), (T, 3, 3))
    et = tt + rng.normal(0, 0.05, (T, 3))
    return tt, tR, et, eR


def _anchor_ranges(wb, i, slot, p, R, off, rng, which=(0, 1, 2, 3)):
    for a in which:
        d = float(np.float32(np.linalg.norm(p + R.apply(off) - ANCH[a]) + rng.normal(0, 0.03)))
        wb.add_range(i, slot, a, d, 1.0 / 0.055 ** 2, off, anchor=True)


def _se3(wb, i, rng, tt, tR, ka, kb, sa, sb, flip=False, robust=True, scale=6e4):
    """a full-information EdgeSE3 between the poses ka -> kb of the trajectory, stored between the slots sa, sb"""
    Zt = tR[ka].inv().apply(tt[kb] - tt[ka]) + rng.normal(0, 0.01, 3)
    ZR = (tR[ka].inv() * tR[kb] * Rotation.from_rotvec(rng.normal(0, 0.01, 3))).as_matrix()
    A = rng.normal(size=(6, 6)); info = A @ A.T + 6 * np.eye(6); info *= scale / np.trace(info)
    if flip: wb.add_se3(i, sb, sa, -ZR.T @ Zt, ZR.T, info, robust)
    else: wb.add_se3(i, sa, sb, Zt, ZR, info, robust)


def fill_chain(wb, i, rng, T, six_dof, loop=False):
    """every pose ranged to all four anchors, smoothness ranges between consecutive poses (some stored the other way round, one link
    missing in some windows); six_dof: a lever arm and an IMU rotation prior per pose; loop: an EdgeSE3 closing 0 <-> T - 1"""
    tt, tR, et, eR = _trajectory(rng, T, six_dof)
    off = LEVER if six_dof else np.zeros(3)
    for k in range(T): wb.add_pose(i, et[k], eR[k])
    for k in range(T):
        _anchor_ranges(wb, i, k, tt[k], tR[k], off, rng)
        if k and not (i % 5 == 2 and k == 3):
            if (i + k) % 3 == 1: wb.add_range(i, k, k - 1, 0.0, SMOOTH_INFO)
            else: wb.add_range(i, k - 1, k, 0.0, SMOOTH_INFO)
        if six_dof:
            wb.add_prior(i, k, et[k], (tR[k] * Rotation.from_rotvec(rng.normal(0, 2e-3, 3))).as_matrix(), IMU_INFO)
        elif k % 2 == 0 and i % 2 == 0:   # a lidar-style z prior (identity rotation, no rotation information)
            wb.add_prior(i, k, np.array([et[k, 0], et[k, 1], tt[k, 2] + rng.normal(0, 0.02)]), np.eye(3), np.array([0, 0, 1 / 0.05, 0, 0, 0.0]))
    if loop:
        _se3(wb, i, rng, tt, tR, T - 1, 0, T - 1, 0, scale=1e3)


def fill_stars(wb, i, rng, T, every, key_first):
    """Key-frame stars as addPoseEdge builds them: groups of `every` poses, each group's key joined to its other poses and to the previous
    group's key by full-information EdgeSE3; the key ranged to all four anchors, every other pose to one.  Slot order inside a group: the
    other poses, then the key (leaves-first, the way loc_node_* packs) or the key, then the other poses (key_first) — the same draws from
    rng either way, so that the two packings of one seed are the SAME star."""
    tt, tR, et, eR = _trajectory(rng, T)
    groups = [list(range(g, min(g + every, T))) for g in range(0, T, every)]
    slot = np.zeros(T, dtype=int)   # slot of trajectory pose k
    keys = []
    for g in groups:
        key = g[-1]
        keys.append(key)
        order = [key] + g[:-1] if key_first else g
        for s, k in zip(range(g[0], g[0] + len(g)), order): slot[k] = s
    inv = np.argsort(slot)
    for s in range(T): wb.add_pose(i, et[inv[s]], eR[inv[s]])
    for n, g in enumerate(groups):
        key = g[-1]
        _anchor_ranges(wb, i, slot[key], tt[key], tR[key], np.zeros(3), rng)
        for k in g[:-1]:
            _anchor_ranges(wb, i, slot[k], tt[k], tR[k], np.zeros(3), rng, which=(k % 4,))
            _se3(wb, i, rng, tt, tR, key, k, slot[key], slot[k], flip=k % 3 == 0, robust=k % 5 != 0)
        if n: _se3(wb, i, rng, tt, tR, keys[n - 1], key, slot[keys[n - 1]], slot[key])


def fill_arrowhead6(wb, i, rng, T, A):
    """a 6-DoF arrowhead: T tag poses (lever arm, IMU priors, smoothness ranges, two surveyed anchors each) that range A unknown anchors,
    the window's last slots (identity rotation, a position prior each: their rotations are excluded)"""
    tt, tR, et, eR = _trajectory(rng, T)
    nodes = np.column_stack([rng.uniform(-4, 4, A), rng.uniform(-4, 4, A), rng.uniform(0, 3, A)])
    for k in range(T): wb.add_pose(i, et[k], eR[k])
    for a in range(A):
        hyp = nodes[a] + rng.normal(0, 0.3, 3)
        wb.add_pose(i, hyp)
        wb.add_prior(i, T + a, hyp, np.eye(3), np.array([1.0, 1.0, 1.0, 0, 0, 0]))
    for k in range(T):
        _anchor_ranges(wb, i, k, tt[k], tR[k], LEVER, rng, which=(k % 4, (k + 1) % 4))
        for a in range(A):
            d = float(np.float32(np.linalg.norm(tt[k] + tR[k].apply(LEVER) - nodes[a]) + rng.normal(0, 0.03)))
            wb.add_range(i, k, T + a, d, 1.0 / 0.055 ** 2, LEVER)
        if k: wb.add_range(i, k - 1, k, 0.0, SMOOTH_INFO)
        wb.add_prior(i, k, et[k], (tR[k] * Rotation.from_rotvec(rng.normal(0, 2e-3, 3))).as_matrix(), IMU_INFO)


def fill_banded(wb, i, rng, T, band=3):
    """a random graph with |i - j| <= band: every pose ranged to all four anchors (lever arm, IMU prior); pose-to-pose ranges and EdgeSE3
    factors between random pairs inside the band, some pairs twice"""
    tt, tR, et, eR = _trajectory(rng, T)
    for k in range(T): wb.add_pose(i, et[k], eR[k])
    for k in range(T):
        _anchor_ranges(wb, i, k, tt[k], tR[k], LEVER, rng)
        wb.add_prior(i, k, et[k], (tR[k] * Rotation.from_rotvec(rng.normal(0, 2e-3, 3))).as_matrix(), IMU_INFO)
        for d in range(1, band + 1):
            j = k - d
            if j < 0 or rng.random() < 0.4:
                continue
            if rng.random() < 0.5:
                meas = float(np.linalg.norm(tt[k] - tt[j]) + rng.normal(0, 0.01))
                if rng.random() < 0.5: wb.add_range(i, k, j, meas, 1 / 0.1 ** 2)
                else: wb.add_range(i, j, k, meas, 1 / 0.1 ** 2)
            else:
                _se3(wb, i, rng, tt, tR, j, k, j, k, flip=rng.random() < 0.3, scale=1e3)
            if rng.random() < 0.2:
                wb.add_range(i, j, k, float(np.linalg.norm(tt[k] - tt[j])), 1 / 0.2 ** 2)


MIXED_NV = (24, 20, 20, 21, 17, 22)   # ragged: chain, star leaves-first, the same star key-first, arrowhead (18 + 3), loop, banded
MIXED_STAR = 1                        # the window test_singular_window cuts loose


def mixed_batch(la, seed=9100):
    wb = la.WindowBatch(6, 24, 200, 30, 80)
    rng = np.random.default_rng(seed)
    fill_chain(wb, 0, rng, MIXED_NV[0], True)
    fill_stars(wb, 1, np.random.default_rng(seed + 1), MIXED_NV[1], MIXED_NV[1], False)
    fill_stars(wb, 2, np.random.default_rng(seed + 1), MIXED_NV[2], MIXED_NV[2], True)
    fill_arrowhead6(wb, 3, rng, MIXED_NV[3] - 3, 3)
    fill_chain(wb, 4, rng, MIXED_NV[4], True, loop=True)
    fill_banded(wb, 5, rng, MIXED_NV[5])
    assert tuple(int(x) for x in wb.counts[:, 0]) == MIXED_NV
    return wb


def chain_batch(la, seed, B, T, six_dof, nv_max=None, ragged=True):
    nv_max = T if nv_max is None else nv_max
    wb = la.WindowBatch(B, nv_max, 5 * nv_max, nv_max, 0)
    rng = np.random.default_rng(seed)
    for i in range(B):
        fill_chain(wb, i, rng, T if (i % 3 != 1 or not ragged) else T - 7, six_dof)
    return wb


def keyframe_batch(la, seed, B, T, every):
    """the node's key-frame window (cfg/uwb_pose.yaml's topology), leaves-first"""
    wb = la.WindowBatch(B, T, T + 3 * (T // every + 1), 0, T + T // every)
    for i in range(B):
        fill_stars(wb, i, np.random.default_rng(seed + i), T, every, False)
    return wb


def tall_star_batch(la, seed):
    """key-first stars of 80 and 71 poses: their first columns hold 79 … 69 rows, either side of the 69 rows up to which
    envelope_covariance_kernel.hip keeps a column in LDS (both of its column paths, and the step from one to the other)"""
    wb = la.WindowBatch(2, 80, 83, 0, 79)
    fill_stars(wb, 0, np.random.default_rng(seed), 80, 80, True)
    fill_stars(wb, 1, np.random.default_rng(seed + 1), 71, 71, True)
    return wb


# The parity cases: name -> (builder, Jacobian modes).  Seeds fixed after the regularity check of tests/test_general_covariance_cpu.py
# passed at the oracle-solved poses.
CASES = {
    "mixed": (lambda la: mixed_batch(la), ("analytic", "numeric")),
    "chain3_65": (lambda la: chain_batch(la, 9201, 3, 65, False), ("analytic", "numeric")),
    "chain3_130": (lambda la: chain_batch(la, 9202, 3, 130, False), ("analytic", "numeric")),
    "chain6_65": (lambda la: chain_batch(la, 9203, 3, 65, True), ("analytic", "numeric")),
    "tall_stars": (lambda la: tall_star_batch(la, 9205), ("analytic", "numeric")),
    "keyframe_300": (lambda la: keyframe_batch(la, 9204, 2, 300, 10), ("numeric",)),
}


def case_batch(la, name):
    return CASES[name][0](la)


# ---- the numpy model of the envelope pass --------------------------------------------------------------------------------------------------
def envelope_first(nv, pairs):
    """first[i]: the smallest slot a pose-to-pose edge joins to slot i (i itself without one)"""
    first = np.arange(nv)
    for u, v in pairs:
        hi, lo = max(u, v), min(u, v)
        first[hi] = min(first[hi], lo)
    return first


def window_pairs(wb, i):
    nr, ns = int(wb.counts[i, 1]), int(wb.counts[i, 3])
    pairs = [(int(wb.r_idx[i, e, 0]), int(wb.r_idx[i, e, 1])) for e in range(nr) if wb.r_idx[i, e, 1] >= 0]
    return pairs + [(int(wb.s_idx[i, e, 0]), int(wb.s_idx[i, e, 1])) for e in range(ns)]


def envelope_blocks(wb, i):
    nv = int(wb.counts[i, 0])
    first = envelope_first(nv, window_pairs(wb, i))
    return int((np.arange(nv) - first + 1).sum())


def envelope_selected_inverse(H, first):
    """The diagonal 6 x 6 blocks of H^-1 the way envelope_covariance_kernel.hip computes them: H [6 nv][6 nv] with every excluded
    coordinate's diagonal set to 1 (rows / columns 0).  Only blocks (i, j) with first[i] <= j <= i are ever read or written; every other
    block of the work arrays is NaN, so that a read outside the envelope poisons the result.  Returns ([nv][6][6], smallest relative pivot)."""
    nv = len(first)
    B = lambda M, i, j: M[6 * i:6 * i + 6, 6 * j:6 * j + 6]
    W = np.full_like(H, np.nan)
    for i in range(nv):
        for j in range(first[i], i + 1):
            B(W, i, j)[:] = B(H, i, j)
    struct = [[k for k in range(j + 1, nv) if first[k] <= j] for j in range(nv)]
    d0 = np.diag(H).copy()
    worst = np.inf
    for j in range(nv):
        S = B(W, j, j).copy()
        L = np.linalg.cholesky((S + S.T) / 2)
        worst = min(worst, (np.diag(L) ** 2 / d0[6 * j:6 * j + 6]).min())   # (the Cholesky pivots of the block = the LDL^T pivots of H)
        Sinv = np.linalg.inv(S)
        col = {k: B(W, k, j).copy() for k in struct[j]}
        for k in struct[j]:
            B(W, k, j)[:] = col[k] @ Sinv
        for a, ka in enumerate(struct[j]):
            for kb in struct[j][:a + 1]:
                assert first[ka] <= kb
                B(W, ka, kb)[:] -= B(W, ka, j) @ col[kb].T
        B(W, j, j)[:] = Sinv
    for j in range(nv - 1, -1, -1):
        sig = lambda i, k: B(W, i, k) if i >= k else B(W, k, i).T
        new = {i: -sum(sig(i, k) @ B(W, k, j) for k in struct[j]) for i in struct[j]}
        B(W, j, j)[:] -= sum((B(W, k, j).T @ new[k] for k in struct[j]), np.zeros((6, 6)))
        for i in struct[j]:
            B(W, i, j)[:] = new[i]
    return np.stack([B(W, v, v) for v in range(nv)]), worst


def min_relative_pivot(H):
    """smallest LDL^T pivot of H_kept relative to its diagonal entry (natural order)"""
    keep = np.diag(H) != 0
    M = H[np.ix_(keep, keep)].copy()
    d0 = np.diag(M).copy()
    worst = np.inf
    for j in range(len(M)):
        worst = min(worst, M[j, j] / d0[j])
        if not M[j, j] > 0:
            return worst
        M[j + 1:, j + 1:] -= np.outer(M[j + 1:, j], M[j, j + 1:]) / M[j, j]
    return worst
