"""GPU checks of the marginal pose covariances of FOREST windows (forest_covariance_kernel.hip through loc_window_covariance_host /
_resident) against the numpy reference of tests/_covariance_ref.py, at the estimates the solve returns.  Definition: DESIGN.md §2,
tolerances and measured values: DESIGN.md §3.

Every input meant to pass is regular by the reference alone: at the oracle-solved poses every LDL^T pivot of H_kept is above 1e-9 of
its diagonal entry (checked on the CPU when the inputs were fixed; test_inputs_are_regular_by_the_reference repeats it at the GPU's
poses), two orders clear of the kernel's 1e-11 rule."""
import numpy as np
import pytest
from scipy.spatial.transform import Rotation

from test_gpu_tree_parity import ANCH, _forest_batch, _rel
from _covariance_ref import hessian, reference_covariance

pytestmark = pytest.mark.gpu

LOC_ERR_UNSUPPORTED, LOC_ERR_SINGULAR = -5, -6
# Frobenius norm of (GPU block - reference block) relative to the reference block's.  analytic: the project's 1e-8.  numeric: 10x the
# largest value measured over every case of this file on an MI355X (8.4e-12, on the 64-pose random forests — their analytic run is at 7.9e-12,
# so it is the conditioning of H, not the difference quotient; DESIGN.md §3 lists every case), capped at 1e-6.
TOL = {"analytic": 1e-8, "numeric": 8.5e-11}


def _random_forest_batch(la, rng, B, T):
    """Forests nobody designed, in the manner of test_tree_wave_kernel_on_random_forests: every pose hangs on a random earlier pose (bushy
    nodes, inner children, chains), two or three trees, smoothness ranges beside some EdgeSE3, priors on a few poses, EdgeSE3 stored in
    either direction — but every tree has at least three poses and every pose 2 … 4 anchor ranges (roots all four), so that H is regular
    without damping.  One topology for the whole batch."""
    while True:
        parent = np.full(T, -1)
        roots = sorted(rng.choice(np.arange(1, T), size=int(rng.integers(1, 3)), replace=False).tolist() + [0])
        for k in range(1, T):
            if k in roots:
                continue
            parent[k] = int(rng.integers(0, k)) if rng.random() < 0.7 else int(rng.choice([0, max(0, k - 1), k // 2]))
        root_of = np.arange(T)
        for k in range(T):
            if parent[k] >= 0:
                root_of[k] = root_of[parent[k]]
        if np.bincount(root_of, minlength=T)[roots].min() >= 3 and np.bincount(parent[parent >= 0], minlength=T).max() >= 4:
            break
    n_anchor = rng.integers(2, 5, T); n_anchor[roots] = 4
    smooth = rng.random(T) < 0.25
    prior = rng.random(T) < 0.15
    flip = rng.random(T) < 0.4
    wb = la.WindowBatch(B, T, 5 * T + 2, T, T)
    for i in range(B):
        tt = np.cumsum(rng.normal(0, 0.08, (T, 3)), axis=0) + np.array([rng.uniform(-1.5, 1.5), rng.uniform(-1.5, 1.5), 1.1])
        tR = Rotation.from_rotvec(np.cumsum(rng.normal(0, 0.03, (T, 3)), axis=0) + rng.normal(0, 0.3, 3))
        et = tt + rng.normal(0, 0.04, (T, 3))
        eR = (tR * Rotation.from_rotvec(rng.normal(0, 0.02, (T, 3)))).as_matrix()
        off = np.array([0.08, -0.02, 0.05])
        for k in range(T): wb.add_pose(i, et[k], eR[k])
        for k in range(T):
            for a in range(int(n_anchor[k])):
                an = (k + a) % 4
                wb.add_range(i, k, an, float(np.float32(np.linalg.norm(tt[k] + tR[k].apply(off) - ANCH[an]) + rng.normal(0, 0.03))), 1 / 0.055 ** 2, off, anchor=True)
            p = int(parent[k])
            if p < 0:
                continue
            Zt = tR[p].inv().apply(tt[k] - tt[p]) + rng.normal(0, 0.01, 3)
            ZR = (tR[p].inv() * tR[k] * Rotation.from_rotvec(rng.normal(0, 0.01, 3))).as_matrix()
            A = rng.normal(size=(6, 6)); info = A @ A.T + 6 * np.eye(6); info *= 6e4 / np.trace(info)
            if flip[k]: wb.add_se3(i, k, p, -ZR.T @ Zt, ZR.T, info, True)
            else: wb.add_se3(i, p, k, Zt, ZR, info, k % 7 != 0)
            if smooth[k]:
                if k % 2: wb.add_range(i, p, k, float(np.linalg.norm(tt[k] - tt[p])), 1 / 0.1 ** 2)
                else: wb.add_range(i, k, p, float(np.linalg.norm(tt[k] - tt[p])), 1 / 0.1 ** 2)
            if prior[k]:
                wb.add_prior(i, k, et[k], (tR[k] * Rotation.from_rotvec(rng.normal(0, 2e-3, 3))).as_matrix(), np.array([0, 0, 0.5, 1, 1, 1.0]) / 4.592449e-06)
    return wb


def _two_trees(wb):
    """_forest_batch's rich (24, 4) windows leave pose T/2 = 12 on its own — no EdgeSE3, one anchor range with a lever arm: six unknowns, rank
    one, H singular by the reference alone.  The inputs are changed, not the check: pose 12 hangs on its key (11) like its neighbours, and
    the link between the keys 11 and 15 goes instead, so that the window still holds two trees — poses 0 … 14 and 15 … 23, each with one
    anchor range per pose, IMU-style priors, doubled pairs and EdgeSE3 in both directions."""
    assert wb.caps[0] == 24
    for i in range(wb.B):
        ns = int(wb.counts[i, 3])
        keep = [e for e in range(ns) if {int(wb.s_idx[i, e, 0]), int(wb.s_idx[i, e, 1])} != {11, 15}]
        assert len(keep) == ns - 1
        wb.s_idx[i, :len(keep)] = wb.s_idx[i, keep].copy(); wb.s_val[i, :len(keep)] = wb.s_val[i, keep].copy()
        wb.counts[i, 3] = len(keep)
        wb.add_se3(i, 11, 12, *_rel(wb, i, 11, 12), np.diag([3e4, 2e4, 1e4, 8e3, 9e3, 1e4]), True)
    return wb


def _isolate_last_pose(wb, rng):
    """The last pose of every window loses its EdgeSE3 (it is a leaf of the last star) and is ranged to all four anchors instead: an isolated
    pose whose translation is determined and whose rotation nothing observes (no lever arm, no prior)."""
    T = wb.caps[0]
    for i in range(wb.B):
        ns = int(wb.counts[i, 3])
        keep = [e for e in range(ns) if T - 1 not in (wb.s_idx[i, e, 0], wb.s_idx[i, e, 1])]
        assert len(keep) == ns - 1
        wb.s_idx[i, :len(keep)] = wb.s_idx[i, keep].copy(); wb.s_val[i, :len(keep)] = wb.s_val[i, keep].copy()
        wb.counts[i, 3] = len(keep)
        have = [int(-1 - wb.r_idx[i, e, 1]) for e in range(int(wb.counts[i, 1])) if wb.r_idx[i, e, 0] == T - 1 and wb.r_idx[i, e, 1] < 0]
        for a in range(4):
            if a not in have:
                wb.add_range(i, T - 1, a, float(np.linalg.norm(wb.poses[i, T - 1, 9:] - ANCH[a]) + rng.normal(0, 0.03)), 1 / 0.055 ** 2, np.zeros(3), anchor=True)
    return wb


def _case(la, name):
    """(batch, kernel the solve takes) of the named parity case"""
    if name == "cfg5_64_8":
        return _forest_batch(la, np.random.default_rng(8100), 8, 64, 8, False), "tree_wave_kernel"
    if name == "rich_24_4":
        return _two_trees(_forest_batch(la, np.random.default_rng(8101), 12, 24, 4, True)), "tree_wave_kernel"
    if name == "rich_10_1":
        return _forest_batch(la, np.random.default_rng(8102), 12, 10, 1, True), None
    if name == "plain_33_5":
        return _forest_batch(la, np.random.default_rng(8103), 12, 33, 5, False), "tree_wave_kernel"
    if name == "doubled_se3":
        wb = _two_trees(_forest_batch(la, np.random.default_rng(8104), 12, 24, 4, True))
        for i in range(wb.B):   # a second EdgeSE3 from a node to its parent: the solve goes to tree_lm_kernel
            wb.add_se3(i, 3, 5, *_rel(wb, i, 3, 5), np.eye(6) * 2e3, True)
        return wb, "tree_lm_kernel"
    if name == "isolated_pose":
        rng = np.random.default_rng(8105)
        return _isolate_last_pose(_forest_batch(la, rng, 12, 24, 4, False), rng), "tree_wave_kernel"
    if name.startswith("random"):
        seed, T = {"random_40": (1, 40), "random_64": (2, 64), "random_33": (3, 33)}[name]
        return _random_forest_batch(la, np.random.default_rng(8200 + seed), 8, T), "tree_wave_kernel"
    raise KeyError(name)


CASES = ["cfg5_64_8", "rich_24_4", "rich_10_1", "plain_33_5", "doubled_se3", "isolated_pose", "random_40", "random_64", "random_33"]
PLAIN = {"cfg5_64_8", "plain_33_5"}   # no lever arm, no rotation prior: the EdgeSE3 factors alone make every rotation observable


def _min_relative_pivot(H):
    """smallest LDL^T pivot of H_kept relative to its diagonal entry (natural order)"""
    keep = np.diag(H) != 0
    A = H[np.ix_(keep, keep)].copy()
    d0 = np.diag(A).copy()
    worst = np.inf
    for j in range(len(A)):
        worst = min(worst, A[j, j] / d0[j])
        if not A[j, j] > 0:
            return worst
        A[j + 1:, j + 1:] -= np.outer(A[j + 1:, j], A[j, j + 1:]) / A[j, j]
    return worst


def _check(O, wb, jac, cov, mask, status):
    mode = O.JAC_ANALYTIC if jac == "analytic" else O.JAC_NUMERIC_G2O
    worst = 0.0
    for i in range(wb.B):
        nv = int(wb.counts[i, 0])
        assert status[i] == 0, (i, status[i])
        assert not cov[i, nv:].any() and not mask[i, nv:].any()
        want, want_mask = reference_covariance(wb, i, ANCH, mode)
        assert np.array_equal(mask[i, :nv], want_mask), (i, mask[i, :nv], want_mask)
        H = hessian(wb, i, ANCH, mode)
        keep = np.diag(H) != 0
        kappa = np.linalg.cond(H[np.ix_(keep, keep)])
        tol = TOL[jac] if kappa <= 1e9 else max(TOL[jac], 1e-15 * kappa)
        for v in range(nv):
            g, r = cov[i, v], want[v]
            nr = np.linalg.norm(r)
            assert nr > 0
            err = np.linalg.norm(g - r) / nr
            worst = max(worst, err)
            assert err <= tol, (i, v, err, tol, kappa)
            assert np.array_equal(g, g.T)
            ev = np.linalg.eigvalsh(g)
            assert ev.min() >= -1e-12 * ev.max()
            for k in range(6):
                if (mask[i, v] >> k) & 1:
                    assert not g[k].any() and not g[:, k].any()
    return worst


@pytest.mark.parametrize("jac", ["analytic", "numeric"])
@pytest.mark.parametrize("name", CASES)
def test_parity_with_the_reference(gpu, name, jac):
    import localization_amd as la
    from oracle import oracle as O
    wb, kernel = _case(la, name)
    T = wb.caps[0]
    s = la.WindowSolver(ANCH, wb.B, *wb.caps, jacobian=jac, bw_max=T - 1, chain_threshold=1)
    s.solve(wb)
    if kernel is not None:
        assert s.last_kernel_kind() == kernel
    cov, mask, status = s.covariance(wb)
    assert s.last_covariance_ms() > 0
    s.close()
    worst = _check(O, wb, jac, cov, mask, status)
    print(f"forest covariance {name} {jac}: max relative Frobenius error {worst:.3e}")
    nv = wb.counts[:, 0]
    if name in PLAIN:
        assert not mask.any()
    if name == "isolated_pose":
        assert (mask[:, T - 1] == 0x38).all() and not mask[:, :T - 1].any()
        assert (nv == T).all()


@pytest.mark.parametrize("name", CASES)
def test_inputs_are_regular_by_the_reference(gpu, name):
    """Every LDL^T pivot of the reference's H_kept is above 1e-9 of its diagonal entry at the solved poses: two orders clear of the 1e-11
    rule, so no window of the parity cases is near the singular verdict."""
    import localization_amd as la
    from oracle import oracle as O
    wb, _ = _case(la, name)
    s = la.WindowSolver(ANCH, wb.B, *wb.caps, jacobian="numeric", bw_max=wb.caps[0] - 1, chain_threshold=1)
    s.solve(wb)
    s.close()
    for i in range(wb.B):
        assert _min_relative_pivot(hessian(wb, i, ANCH, O.JAC_NUMERIC_G2O)) > 1e-9, i


def test_singular_window_is_isolated(gpu):
    """One window of a plain batch keeps its structure but loses the information of all its range edges: a gauge-free tree, H singular —
    LOC_ERR_SINGULAR and NaN; the other windows are bit-identical to the batch without the change."""
    import localization_amd as la
    B, T = 9, 24
    wb = _forest_batch(la, np.random.default_rng(8300), B, T, 4, False)
    s = la.WindowSolver(ANCH, B, *wb.caps, jacobian="numeric", bw_max=T - 1, chain_threshold=1)
    s.solve(wb)
    cov0, mask0, st0 = s.covariance(wb)
    assert (st0 == 0).all()
    bad = wb.copy()
    i = 4
    bad.r_val[i, :, 1] = 0.0
    cov, mask, st = s.covariance(bad)
    s.close()
    assert st[i] == LOC_ERR_SINGULAR and np.isnan(cov[i]).all()
    others = [k for k in range(B) if k != i]
    assert (st[others] == 0).all()
    assert np.array_equal(cov[others], cov0[others]) and np.array_equal(mask[others], mask0[others])


@pytest.mark.parametrize("kernel", ["tree_wave_kernel", "tree_lm_kernel"])
def test_resident_matches_host_bit_for_bit(gpu, kernel):
    import torch
    import localization_amd as la
    B, T = 300, 24
    wb = _two_trees(_forest_batch(la, np.random.default_rng(8400), B, T, 4, True))
    if kernel == "tree_lm_kernel":
        for i in range(B):
            wb.add_se3(i, 3, 5, *_rel(wb, i, 3, 5), np.eye(6) * 2e3, True)
    s = la.WindowSolver(ANCH, B, *wb.caps, jacobian="numeric", bw_max=T - 1)   # (the default rule: 300 windows are a forest batch)
    s.upload(wb)
    s.solve_resident()
    assert s.last_kernel_kind() == kernel

    def fresh():
        return (torch.full((B, T, 6, 6), 7.0, dtype=torch.float64, device=gpu), torch.full((B, T), 7, dtype=torch.int32, device=gpu),
                torch.full((B,), 7, dtype=torch.int32, device=gpu))

    cov_d, mask_d, st_d = fresh()
    s.covariance_resident(cov_d, mask_d, st_d)
    assert s.last_covariance_ms() > 0
    other = torch.cuda.Stream(device=gpu)
    cov_e, mask_e, st_e = fresh()
    torch.cuda.synchronize()
    s.covariance_resident(cov_e, mask_e, st_e, stream=other)
    other.synchronize()
    s.download(wb)
    cov, mask, st = s.covariance(wb)
    for c, m, t in ((cov_d, mask_d, st_d), (cov_e, mask_e, st_e)):
        assert np.array_equal(c.cpu().numpy(), cov) and np.array_equal(m.cpu().numpy(), mask) and np.array_equal(t.cpu().numpy(), st)
    assert (st == 0).all()
    # the resident batch is still there: another solve + download gives the same poses
    before = wb.poses.copy()
    s.solve_resident()
    s.download(wb)
    assert s.last_kernel_kind() == kernel and np.array_equal(wb.poses, before)
    s.close()


def test_solves_are_unaffected(gpu):
    """A handle that computes covariances between its solves — of the batch it solves (a topology-cache hit on the host path) and of a forest
    with ANOTHER topology — returns the same bits (poses, results, kernel kind) as one that never does, on the host path and resident."""
    import torch
    import localization_amd as la
    B, T = 16, 24
    wb = _forest_batch(la, np.random.default_rng(8500), B, T, 4, True)
    other = _forest_batch(la, np.random.default_rng(8501), B, T, 6, False)
    a = la.WindowSolver(ANCH, B, *wb.caps, bw_max=T - 1, chain_threshold=1)
    b = la.WindowSolver(ANCH, B, *wb.caps, bw_max=T - 1, chain_threshold=1)
    wa, wc = wb.copy(), wb.copy()
    for rep in range(3):
        ra = a.solve(wa).copy()
        a.covariance(wa)
        a.covariance(other)
        rb = b.solve(wc).copy()
        assert np.array_equal(wa.poses, wc.poses) and np.array_equal(ra, rb)
        assert a.last_kernel_kind() == b.last_kernel_kind() == "tree_wave_kernel"
        wa.poses[:, :, 9:] += 0.01; wc.poses[:, :, 9:] += 0.01
    wa, wc = wb.copy(), wb.copy()
    a.upload(wa); b.upload(wc)
    out = (torch.zeros((B, T, 36), dtype=torch.float64, device=gpu), torch.zeros((B, T), dtype=torch.int32, device=gpu), torch.zeros((B,), dtype=torch.int32, device=gpu))
    for rep in range(2):
        a.solve_resident(); b.solve_resident()
        a.covariance_resident(*out)
        a.covariance(other)
        ra, rb = a.download(wa).copy(), b.download(wc).copy()
        assert np.array_equal(wa.poses, wc.poses) and np.array_equal(ra, rb)
        assert a.last_kernel_kind() == b.last_kernel_kind() == "tree_wave_kernel"
    a.close(); b.close()


def test_coverage_rule(gpu):
    """Served iff the handle would solve the batch on a structured kernel: chains as before, forests under the tree kernels' own rule."""
    import localization_amd as la
    from test_gpu_covariance import _twist_batch
    rng = np.random.default_rng(8600)
    T = 12

    def untouched(s, wb):
        out = (np.full((wb.B, wb.caps[0], 6, 6), 7.0), np.full((wb.B, wb.caps[0]), 7, dtype=np.int32), np.full(wb.B, 7, dtype=np.int32))
        with pytest.raises(la.LocalizationAmdError) as ex:
            s.covariance(wb, out=out)
        assert ex.value.code == LOC_ERR_UNSUPPORTED
        assert (out[0] == 7.0).all() and (out[1] == 7).all() and (out[2] == 7).all()

    wb = _forest_batch(la, rng, 2, T, 4, False)
    s = la.WindowSolver(ANCH, 2, *wb.caps, bw_max=T - 1)
    s.solve(wb)
    untouched(s, wb)                                   # default handle: two windows are no forest batch
    s.close()
    s = la.WindowSolver(ANCH, 2, *wb.caps, bw_max=T - 1, chain_threshold=1)
    cov, mask, st = s.covariance(wb)                   # the same batch with the threshold lowered: served
    assert (st == 0).all() and np.isfinite(cov).all() and cov[:, :, 0, 0].all()
    s.set_option("tree", 0)
    untouched(s, wb)                                   # the forest kernels switched off
    s.set_option("tree", -1)
    odd = wb.copy()
    odd.r_idx[1, 3, 1] = -1 - 2                        # one window ranges another anchor: not ONE topology
    untouched(s, odd)
    s.close()
    big = _forest_batch(la, rng, 2, 65, 8, False)      # more than 64 poses
    s = la.WindowSolver(ANCH, 2, *big.caps, bw_max=64, chain_threshold=1)
    untouched(s, big)
    s.close()
    # a chain batch still runs the chain pass: the same bits as on a handle whose forest kernels are off
    # (test_gpu_covariance.test_six_dof_chains' fifteen-pose twist windows, its generator and handle: regular there)
    ch = _twist_batch(la, np.random.default_rng(500 + 15 + len("twist_robust") + len("numeric")), 24, 15, True)
    a, b = la.WindowSolver(ANCH, 24, *ch.caps, jacobian="numeric"), la.WindowSolver(ANCH, 24, *ch.caps, jacobian="numeric")
    b.set_option("tree", 0)
    a.solve(ch)
    ca, cb = a.covariance(ch), b.covariance(ch)
    assert (ca[2] == 0).all() and all(np.array_equal(x, y) for x, y in zip(ca, cb))
    c = la.WindowSolver(ANCH, 24, *ch.caps, jacobian="numeric", chain_threshold=1)   # takes forests from one window on: the chain test still comes first
    cc = c.covariance(ch)
    assert all(np.array_equal(x, y) for x, y in zip(cc, cb))
    c.close()
    a.close(); b.close()
