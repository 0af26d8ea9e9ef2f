"""dev: wave3_lm_kernel / wave6_lm_kernel against the general wave-per-window kernel on thousands of random chain windows (random
lengths 1 .. 64, missing links, ranges with zero information, far-off initial estimates, lidar-style second priors): analytic mode,
so the two agree to ~1e-7 m unless an LM accept / reject decision flips on a rounding-level difference."""
import os, sys
import numpy as np
from scipy.spatial.transform import Rotation
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import localization_amd as la

ANCH = np.array([[3, -3, 0.58], [3, 3, 1.97], [-3, 3, 0.54], [-3, -3, 1.76]], dtype=float)


def build(B, Tmax, six, seed):
    rng = np.random.default_rng(seed)
    wb = la.WindowBatch(B, Tmax, 3 * Tmax + 4, (2 * Tmax if six else Tmax), 0)
    for i in range(B):
        T = int(rng.integers(1, Tmax + 1))
        truth = np.cumsum(rng.normal(0, 0.05, (T, 3)), axis=0) + np.array([rng.uniform(-1.5, 1.5), rng.uniform(-1.5, 1.5), 1.1])
        est = truth + rng.normal(0, 0.05 if i % 11 else 0.6, (T, 3))          # (some windows start far off: rejected trials)
        tR = Rotation.from_rotvec(np.cumsum(rng.normal(0, 0.03, (T, 3)), axis=0) + rng.normal(0, 0.3, 3)) if six else None
        off = np.array([0.1, 0.0, -0.05]) if six else np.zeros(3)
        for k in range(T):
            if six: wb.add_pose(i, est[k], (tR[k] * Rotation.from_rotvec(rng.normal(0, 0.02, 3))).as_matrix())
            else: wb.add_pose(i, est[k])
        for k in range(T):
            for a in rng.choice(4, size=int(rng.integers(1, 3)), replace=False):
                p = truth[k] + (tR[k].apply(off) if six else 0.0)
                info = 0.0 if rng.random() < 0.02 else 1.0 / 0.055 ** 2
                wb.add_range(i, k, int(a), float(np.float32(np.linalg.norm(p - ANCH[a]) + rng.normal(0, 0.03))), info, off, anchor=True)
            if k > 0 and rng.random() > 0.05:
                if rng.random() < 0.5: wb.add_range(i, k - 1, k, 0.0, 1.0 / (5.0 / 32 / 3) ** 2)
                else: wb.add_range(i, k, k - 1, 0.0, 1.0 / (5.0 / 32 / 3) ** 2)
            if six:
                wb.add_prior(i, k, est[k], (tR[k] * Rotation.from_rotvec(rng.normal(0, 2e-3, 3))).as_matrix(), np.array([0, 0, 0, 1, 1, 1.0]) / 4.592449e-06)
                if rng.random() < 0.3: wb.add_prior(i, k, est[k] + np.array([0, 0, rng.normal(0, 0.02)]), np.eye(3), np.array([0, 0, 20.0, 0, 0, 0]))
            elif rng.random() < 0.2:
                wb.add_prior(i, k, est[k] + np.array([0, 0, rng.normal(0, 0.02)]), np.eye(3), np.array([0, 0, 20.0, 0, 0, 0]))
    return wb


for six, B, Tmax in ((False, 8192, 64), (False, 8192, 12), (True, 4096, 40), (True, 4096, 12)):
    wb = build(B, Tmax, six, 17 + Tmax)
    ref = wb.copy()
    g = la.WindowSolver(ANCH, B, *wb.caps, jacobian="analytic", chain_threshold=0)
    rg = g.solve(ref).copy(); kg = g.last_kernel_kind(); g.close()
    s = la.WindowSolver(ANCH, B, *wb.caps, jacobian="analytic")
    rs = s.solve(wb).copy(); ks = s.last_kernel_kind(); s.close()
    d = np.zeros(B)
    for i in range(B):
        nv = int(wb.counts[i, 0]); d[i] = np.abs(wb.poses[i, :nv] - ref.poses[i, :nv]).max() if nv else 0.0
    same_trials = (rs[:, 4] == rg[:, 4])
    print(f"{ks} vs {kg}: B={B} Tmax={Tmax}: max |dpose| {d.max():.2e}, median {np.median(d):.1e}, > 1e-6: {(d > 1e-6).sum()}; trial counts differ in {(~same_trials).sum()}, "
          f"terminated differs in {(rs[:, 5] != rg[:, 5]).sum()}; among windows with equal trial counts max |dpose| {d[same_trials].max():.2e}, chi2 rel {np.abs(rs[same_trials, 0] - rg[same_trials, 0]).max() / max(1.0, np.abs(rg[:, 0]).max()):.1e}")

# the windows where the two kernels differ most: which one is closer to the oracle?
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _oracle_window import oracle_solve_instance
wb = build(8192, 64, False, 17 + 64)
ref = wb.copy(); orig = wb.copy()
g = la.WindowSolver(ANCH, 8192, *wb.caps, jacobian="analytic", chain_threshold=0); g.solve(ref); g.close()
s = la.WindowSolver(ANCH, 8192, *wb.caps, jacobian="analytic"); rs = s.solve(wb).copy(); s.close()
d = np.array([np.abs(wb.poses[i, :int(wb.counts[i, 0])] - ref.poses[i, :int(wb.counts[i, 0])]).max() for i in range(8192)])
for i in np.argsort(d)[-6:]:
    nv = int(wb.counts[i, 0])
    poses, chi, st = oracle_solve_instance(orig, int(i), ANCH)
    print(f"window {i}: nv {nv}, wave3 vs general {d[i]:.2e}; wave3 vs oracle {np.abs(wb.poses[i, :nv] - poses).max():.2e}; general vs oracle {np.abs(ref.poses[i, :nv] - poses).max():.2e}; "
          f"trials {int(rs[i, 4])} (oracle {st.lm_trials}), lambda {rs[i, 2]:.2e}")
