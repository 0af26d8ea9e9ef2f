"""Test helper of tests/test_gpu_forest_groups.py: batches of forest windows whose topologies DIFFER (option "forest_groups").  A topology
is described once (parents, storage directions, edge counts per pose); every window of that topology gets its own measurements, its own
estimates and — `vary` — its own anchor choice and robust flags, which are not part of a topology."""
import numpy as np
from scipy.spatial.transform import Rotation

ANCH = np.array([[3, -3, 0.58], [3, 3, 1.97], [-3, 3, 0.54], [-3, -3, 1.76]], dtype=float)   # tests/test_gpu_tree_parity.py's
CAPS = (64, 136, 64, 64)     # nv_max, nr_max, np_max, ns_max of every batch here (nr: the random forest's up to four ranges per pose)


def star(T, every, rich=False, first=None, n_anchor=1, lever=False, reverse=False, prior_on=()):
    """A key-frame star as Localization::addPoseEdge builds it and tests/test_gpu_tree_parity.py: _forest_batch writes it: a new key every
    `every` poses, the pose before a new key IS that key.  first: the length of the first key run (the phase of the cadence; default `every`).
    rich: two trees (pose T/2 hangs on nothing), a smoothness range next to the EdgeSE3 where the key is the previous pose, priors on
    every fourth pose, lever arms, EdgeSE3 stored in either direction, some not robust.  reverse: the poses' edges are created from the last
    pose down (edges not in the order of their later pose: no ORDERED chain, whatever the graph).  prior_on: poses with an IMU-style prior."""
    first = every if first is None else first
    k = np.arange(T)
    parent = np.where(k < first, 0, ((k - first) // every) * every + first - 1)
    parent[0] = -1
    if rich:
        parent[T // 2] = -1
    return dict(T=T, parent=parent, flip=rich & (k % 3 == 0), robust=~(rich & (k % 5 == 0) & (k % 3 != 0)), n_anchor=np.full(T, n_anchor),
                smooth=rich & (parent == k - 1), smooth_dir=np.zeros(T, bool), prior=(rich & (k % 4 == 1)) | np.isin(k, list(prior_on)), off=np.array([0.1, 0.0, -0.05]) if rich or lever else np.zeros(3),
                prior_diag=np.array([0, 0, 0, 1, 1, 1.0]) / 4.592449e-06, step=0.05, start=0.05, order=k[::-1] if reverse else k)


def random_forest(T, seed):
    """the recipe of tests/test_gpu_tree_parity.py: test_tree_wave_kernel_on_random_forests: every pose hangs on a random earlier pose, two or
    three trees, 1 .. 3 anchor ranges per pose (roots three), smoothness ranges in either direction, priors, EdgeSE3 in either direction"""
    rng = np.random.default_rng(900 + seed)
    parent = np.full(T, -1)
    roots = sorted(rng.choice(np.arange(1, T), size=int(rng.integers(1, 3)), replace=False).tolist() + [0])
    for k in range(1, T):
        if k not in roots:
            parent[k] = int(rng.integers(0, k)) if rng.random() < 0.7 else int(rng.choice([0, max(0, k - 1), k // 2]))
    n_anchor = rng.integers(1, 4, T); n_anchor[roots] = 3
    k = np.arange(T)
    return dict(T=T, parent=parent, flip=rng.random(T) < 0.4, robust=k % 7 != 0, n_anchor=n_anchor, smooth=(rng.random(T) < 0.25) & (parent >= 0), smooth_dir=k % 2 == 1,
                prior=rng.random(T) < 0.15, off=np.array([0.08, -0.02, 0.05]), prior_diag=np.array([0, 0, 0.5, 1, 1, 1.0]) / 4.592449e-06, step=0.08, start=0.04, order=k)


def five_topologies():
    """the common shape of the GPU tests: (T = 64, key every 8) — (T = 24, every 4, rich) — (T = 40, every 6, a first key run of 2) — (T = 2: one
    EdgeSE3, the smallest forest; three anchor ranges per pose, a lever arm and an IMU-style rotation prior on pose 1 — the ranges fix the two
    antennas, and with them everything but the rotation of the pair about the line that joins them: without the prior that direction is
    unobserved and no two solvers agree along it; its edges created from the
    last pose down — two poses in creation order are an ordered CHAIN, which a batch of such windows alone would take to the chain kernels, not
    to tree_wave_kernel) — a random forest, T = 33"""
    return [star(64, 8), star(24, 4, rich=True), star(40, 6, first=2), star(2, 1, n_anchor=3, lever=True, reverse=True, prior_on=(1,)), random_forest(33, 3)]


def fill_window(wb, i, topo, rng, shift=0, flip_robust=False):
    """window i of wb: topology `topo`, measurements and estimates from rng.  shift: pose k's a-th anchor range goes to anchor (k + a + shift) % 4;
    flip_robust: the robust flag of the window's first EdgeSE3 is inverted.  The stream of random numbers drawn does not depend on either."""
    T, parent, off = topo["T"], topo["parent"], topo["off"]
    tt = np.cumsum(rng.normal(0, topo["step"], (T, 3)), axis=0) + np.array([rng.uniform(-1.5, 1.5), rng.uniform(-1.5, 1.5), 1.1])
    tR = Rotation.from_rotvec(np.cumsum(rng.normal(0, 0.03, (T, 3)), axis=0) + rng.normal(0, 0.3, 3))
    et = tt + rng.normal(0, topo["start"], (T, 3))
    eR = (tR * Rotation.from_rotvec(rng.normal(0, 0.02, (T, 3)))).as_matrix()
    for k in range(T):
        wb.add_pose(i, et[k], eR[k])
    first_se3 = True
    for k in topo["order"].tolist():
        for a in range(int(topo["n_anchor"][k])):
            an = (k + a + shift) % 4
            wb.add_range(i, k, an, float(np.float32(np.linalg.norm(tt[k] + tR[k].apply(off) - ANCH[an]) + rng.normal(0, 0.03))), 1 / 0.055 ** 2, off, anchor=True)
        p = int(parent[k])
        if p < 0:
            continue
        Zt = tR[p].inv().apply(tt[k] - tt[p]) + rng.normal(0, 0.01, 3)
        ZR = (tR[p].inv() * tR[k] * Rotation.from_rotvec(rng.normal(0, 0.01, 3))).as_matrix()
        A = rng.normal(size=(6, 6)); info = A @ A.T + 6 * np.eye(6); info *= 6e4 / np.trace(info)
        robust = bool(topo["robust"][k]) != (flip_robust and first_se3)
        first_se3 = False
        if topo["flip"][k]:
            wb.add_se3(i, k, p, -ZR.T @ Zt, ZR.T, info, robust)              # stored child -> parent: the inverse measurement
        else:
            wb.add_se3(i, p, k, Zt, ZR, info, robust)
        if topo["smooth"][k]:
            v0, v1 = (p, k) if topo["smooth_dir"][k] or p == k - 1 else (k, p)
            wb.add_range(i, v0, v1, float(np.linalg.norm(tt[k] - tt[p])) if topo["step"] > 0.05 else 0.0, 1 / 0.1 ** 2)
        if topo["prior"][k]:
            wb.add_prior(i, k, et[k], (tR[k] * Rotation.from_rotvec(rng.normal(0, 2e-3, 3))).as_matrix(), topo["prior_diag"])


def mixed_batch(la, topos, of, seed, vary=True):
    """window b has topology topos[of[b]].  vary: anchor choice (and, for every third window, one robust flag) differ from window to window;
    else every window of a topology ranges the same anchors — the SAME random stream either way, so that the two batches differ in nothing else
    but the ranged anchors' measurements"""
    wb = la.WindowBatch(len(of), *CAPS)
    rng = np.random.default_rng(seed)
    for b in range(len(of)):
        fill_window(wb, b, topos[of[b]], rng, shift=(b // len(topos)) % 4 if vary else 0, flip_robust=vary and b % 3 == 1)
    return wb
