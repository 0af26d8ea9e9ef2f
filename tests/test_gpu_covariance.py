"""GPU checks of the marginal pose covariances (covariance_kernel.hip through loc_window_covariance_host / _resident) against the numpy
reference of tests/_covariance_ref.py, at the estimates the solve returns.  Definition and tolerances: DESIGN.md §2 / §3."""
import numpy as np
import pytest

from test_gpu_chain3_parity import _translation_only_batch
from test_gpu_wave6_parity import _chain_batch
from test_gpu_window_parity import ANCH, _random_window
from _covariance_ref import reference_covariance

pytestmark = pytest.mark.gpu

LOC_ERR_UNSUPPORTED, LOC_ERR_SINGULAR = -5, -6
# Frobenius norm of (GPU block - reference block) relative to the reference block's; numeric: 10x the largest value measured over
# every case of this file (measured on an MI355X: 1.5e-10, on 15-pose twist windows — their analytic run is at 1.2e-10 as well, so it is the
# conditioning of H, not the difference quotient)
TOL = {"analytic": 1e-8, "numeric": 1.5e-9}


def _observable_batch(la, rng, B, T, imu, lever, lidar=False, translation_only=False):
    """Chain windows whose undamped H is regular: every pose ranged to all four anchors (the reference's stream ranges ONE anchor per
    pose: 2T - 1 rank-one terms for 3T translations — such windows are singular without the LM damping), smoothness
    edges (some stored the other way round, some missing), optionally IMU rotation priors and lidar z priors.  Edges in the order
    Localization::addRangeEdge creates them (a pose's ranges, then its smoothness edge to the previous pose), priors by pose: the batch
    takes the chain solve kernels (wave3 / wave6) as the node's windows do."""
    nr_max, np_max = 5 * T, 2 * T
    wb = la.WindowBatch(B, T, nr_max, np_max, 0)
    for i in range(B):
        Ti = T if i % 7 else max(T // 2, 1)
        est_t, est_R, off, ranges, smooth, priors, _ = _random_window(rng, Ti, imu, False, lever)
        if translation_only:
            est_R = np.broadcast_to(np.eye(3), (Ti, 3, 3))
        for k in range(Ti):
            wb.add_pose(i, est_t[k], est_R[k])
        for k in range(Ti):
            for a in range(4):
                d = float(np.float32(np.linalg.norm(est_t[k] + est_R[k] @ off - ANCH[a]) + rng.normal(0, 0.03)))
                wb.add_range(i, k, a, d, 1.0 / 0.055 ** 2, off, anchor=True)
            for (k0, k1, d, info) in smooth:
                if k1 == k and not (i % 5 == 2 and k1 == 3):   # (some windows miss a link: two independent chains)
                    if i % 3 == 1: wb.add_range(i, k1, k0, d, info)
                    else: wb.add_range(i, k0, k1, d, info)
        for (k, t, R, dg) in priors:
            wb.add_prior(i, k, t, R, dg)
            if lidar and k % 2 == 0:
                wb.add_prior(i, k, np.array([est_t[k, 0], est_t[k, 1], est_t[k, 2] + rng.normal(0, 0.02)]), est_R[k], np.array([0, 0, 1 / 0.05, 0, 0, 0.0]))
        if translation_only and i % 2 == 0:
            for k in range(0, Ti, 2):   # a lidar-style z prior (identity rotation, no rotation information)
                wb.add_prior(i, k, np.array([est_t[k, 0], est_t[k, 1], est_t[k, 2] + rng.normal(0, 0.02)]), np.eye(3), np.array([0, 0, 1 / 0.05, 0, 0, 0.0]))
    return wb


def _twist_batch(la, rng, B, T, robust):
    """cfg/uwb_twist.yaml's window: per pose an anchor range (lever arm), an EdgeSE3 to the previous pose (robust or not), ragged lengths."""
    wb = la.WindowBatch(B, T, 2 * T, 0, T)
    for i in range(B):
        Ti = T if i % 5 else max(T // 2, 1)
        est_t, est_R, off, ranges, smooth, _, _ = _random_window(rng, Ti, False, False, True)
        for k in range(Ti):
            wb.add_pose(i, est_t[k], est_R[k])
        for (k, a, d, info) in ranges:
            wb.add_range(i, k, a, d, info, off, anchor=True)
        for k in range(1, Ti):
            Zt = est_R[k - 1].T @ (est_t[k] - est_t[k - 1]) + rng.normal(0, 0.01, 3)
            A = rng.normal(size=(6, 6)); info = A @ A.T + 6 * np.eye(6); info *= 1e3 / np.trace(info)
            wb.add_se3(i, k - 1, k, Zt, est_R[k - 1].T @ est_R[k], info, robust=robust if i % 2 else not robust)
    return wb


def _check(la, O, wb, jac, cov, mask, status, rot_excluded=None):
    mode = O.JAC_ANALYTIC if jac == "analytic" else O.JAC_NUMERIC_G2O
    worst = 0.0
    for i in range(wb.B):
        nv = int(wb.counts[i, 0])
        assert status[i] == 0
        assert not cov[i, nv:].any() and not mask[i, nv:].any()
        want, want_mask = reference_covariance(wb, i, ANCH, mode)
        assert np.array_equal(mask[i, :nv], want_mask), (i, mask[i, :nv], want_mask)
        for v in range(nv):
            g, r = cov[i, v], want[v]
            nr = np.linalg.norm(r)
            if nr == 0:
                assert not g.any()
                continue
            worst = max(worst, np.linalg.norm(g - r) / nr)
            assert np.array_equal(g, g.T)
            ev = np.linalg.eigvalsh(g)
            assert ev.min() >= -1e-12 * ev.max()
            for k in range(6):
                if (mask[i, v] >> k) & 1:
                    assert not g[k].any() and not g[:, k].any()
    assert worst <= TOL[jac], worst
    print(f"covariance {jac}: max relative Frobenius error {worst:.3e}")
    return worst


@pytest.mark.parametrize("T", [1, 10, 64])
@pytest.mark.parametrize("jac", ["analytic", "numeric"])
def test_translation_only_chains(gpu, T, jac):
    import localization_amd as la
    from oracle import oracle as O
    rng = np.random.default_rng(300 + T + len(jac))
    B = 48 if T < 64 else 12
    wb = _observable_batch(la, rng, B, T, False, False, translation_only=True)
    s = la.WindowSolver(ANCH, B, *wb.caps, jacobian=jac)
    s.solve(wb)
    cov, mask, status = s.covariance(wb)
    for i in range(B):
        nv = int(wb.counts[i, 0])
        assert ((mask[i, :nv] & 0x38) == 0x38).all()
        assert not cov[i, :, 3:, :].any() and not cov[i, :, :, 3:].any()
    _check(la, O, wb, jac, cov, mask, status)


@pytest.mark.parametrize("T,kind,jac", [
    (12, "imu_lever", "analytic"), (12, "imu_lever", "numeric"),
    (16, "imu_lever", "numeric"), (40, "imu", "analytic"), (63, "imu_lever", "numeric"),
    (20, "lidar", "numeric"), (20, "lidar", "analytic"),
    (15, "twist_robust", "numeric"), (15, "twist_plain", "analytic"), (63, "twist_robust", "analytic"),
])
def test_six_dof_chains(gpu, T, kind, jac):
    import localization_amd as la
    from oracle import oracle as O
    rng = np.random.default_rng(500 + T + len(kind) + len(jac))
    B = 24 if T <= 20 else 6
    if kind.startswith("twist"):
        wb = _twist_batch(la, rng, B, T, kind == "twist_robust")
    else:
        wb = _observable_batch(la, rng, B, T, True, kind != "imu", lidar=kind == "lidar")
    s = la.WindowSolver(ANCH, B, *wb.caps, jacobian=jac)
    s.solve(wb)
    cov, mask, status = s.covariance(wb)
    _check(la, O, wb, jac, cov, mask, status)


def test_rotations_without_prior_are_excluded(gpu):
    """No lever arm, IMU priors on only some poses: exactly the rotations of the poses without a prior are excluded."""
    import localization_amd as la
    from oracle import oracle as O
    rng = np.random.default_rng(77)
    B, T = 16, 12
    wb = _observable_batch(la, rng, B, T, True, False)
    # drop the priors of every third pose
    for i in range(B):
        keep = [e for e in range(int(wb.counts[i, 2])) if wb.p_idx[i, e] % 3 != 1]
        wb.p_idx[i, :len(keep)] = wb.p_idx[i, keep].copy(); wb.p_val[i, :len(keep)] = wb.p_val[i, keep].copy()
        wb.counts[i, 2] = len(keep)
    s = la.WindowSolver(ANCH, B, *wb.caps, jacobian="numeric")
    s.solve(wb)
    cov, mask, status = s.covariance(wb)
    for i in range(B):
        for v in range(int(wb.counts[i, 0])):
            assert mask[i, v] == (0x38 if v % 3 == 1 else 0), (i, v, mask[i, v])
    _check(la, O, wb, "numeric", cov, mask, status)


def test_singular_window_is_isolated(gpu):
    """A window whose only pose is joined to nothing but one range (rank-1 H with a lever arm: its second pivot is rounding noise, far
    below the relative threshold whatever its sign) gets LOC_ERR_SINGULAR and NaN; its neighbours are bit-identical to the same batch
    without it."""
    import localization_amd as la
    rng = np.random.default_rng(11)
    B, T = 9, 12
    wb = _observable_batch(la, rng, B, T, True, True)
    s = la.WindowSolver(ANCH, B, *wb.caps, jacobian="numeric")
    s.solve(wb)
    cov0, mask0, st0 = s.covariance(wb)
    bad = wb.copy()
    i = 4
    bad.counts[i] = (1, 1, 0, 0)
    bad.r_idx[i, 0] = (0, -1 - 1); bad.r_val[i, 0] = (3.0, 100.0, 0.1, 0.0, -0.05)
    cov, mask, st = s.covariance(bad)
    assert st[i] == LOC_ERR_SINGULAR and np.isnan(cov[i, 0]).all() and not cov[i, 1:].any()
    others = [k for k in range(B) if k != i]
    assert (st[others] == 0).all()
    assert np.array_equal(cov[others], cov0[others]) and np.array_equal(mask[others], mask0[others])
    # a window whose H is not finite: the same verdict
    bad.r_val[i, 0, 0] = np.nan
    cov, mask, st = s.covariance(bad)
    assert st[i] == LOC_ERR_SINGULAR and np.isnan(cov[i, 0]).all() and np.array_equal(cov[others], cov0[others])


def test_unsupported_structures_write_nothing(gpu):
    import localization_amd as la
    rng = np.random.default_rng(5)

    def untouched(s, wb):
        out = (np.full((wb.B, wb.caps[0], 6, 6), 7.0), np.full((wb.B, wb.caps[0]), 7, dtype=np.int32), np.full(wb.B, 7, dtype=np.int32))
        with pytest.raises(la.LocalizationAmdError) as ex:
            s.covariance(wb, out=out)
        assert ex.value.code == LOC_ERR_UNSUPPORTED
        assert (out[0] == 7.0).all() and (out[1] == 7).all() and (out[2] == 7).all()

    # key-frame star (EdgeSE3 from a key pose to poses further away)
    wb = la.WindowBatch(2, 12, 24, 0, 12)
    for i in range(2):
        est_t, est_R, off, ranges, smooth, priors, se3 = _random_window(rng, 12, False, True, False)
        for k in range(12):
            wb.add_pose(i, est_t[k], est_R[k])
        for (k, a, d, info) in ranges:
            wb.add_range(i, k, a, d, info, anchor=True)
        for (k0, k1, Zt, ZR, info) in se3:
            wb.add_se3(i, k0, k1, Zt, ZR, info)
    untouched(la.WindowSolver(ANCH, 2, *wb.caps), wb)
    # arrowhead: a range from every pose to the last pose slot
    wb = la.WindowBatch(2, 10, 30, 0, 0)
    for i in range(2):
        for k in range(10):
            wb.add_pose(i, rng.normal(0, 1, 3))
        for k in range(9):
            wb.add_range(i, k, int(rng.integers(0, 4)), 2.0, 100.0, anchor=True)
            if k:
                wb.add_range(i, k - 1, k, 0.0, 100.0)
            wb.add_range(i, k, 9, 1.0, 100.0)
    untouched(la.WindowSolver(ANCH, 2, *wb.caps), wb)
    # more than 64 poses
    wb = _translation_only_batch(la, rng, 2, 65, False)
    untouched(la.WindowSolver(ANCH, 2, *wb.caps), wb)
    # lever arms on endpoint 1
    wb = _translation_only_batch(la, rng, 2, 10, False)
    wb.r_off1 = np.zeros((2, wb.caps[1], 3)); wb.r_off1[:, :, 0] = 0.1
    untouched(la.WindowSolver(ANCH, 2, *wb.caps), wb)


def test_resident_matches_host_bit_for_bit(gpu):
    """covariance_resident after upload + solve_resident = covariance(wb) on the downloaded poses, B = 4096 ten-pose translation-only
    windows (cfg/uwb_only.yaml's shape, every pose ranged to all four anchors)."""
    import torch
    import localization_amd as la
    rng = np.random.default_rng(21)
    B, T = 4096, 10
    wb = _observable_batch(la, rng, B, T, False, False, translation_only=True)
    s = la.WindowSolver(ANCH, B, *wb.caps, jacobian="numeric")
    s.upload(wb)
    s.solve_resident()
    cov_d = torch.full((B, T, 6, 6), 7.0, dtype=torch.float64, device=gpu)
    mask_d = torch.full((B, T), 7, dtype=torch.int32, device=gpu)
    st_d = torch.full((B,), 7, dtype=torch.int32, device=gpu)
    s.covariance_resident(cov_d, mask_d, st_d)
    s.download(wb)
    assert s.last_covariance_ms() > 0
    cov, mask, st = s.covariance(wb)
    assert np.array_equal(cov_d.cpu().numpy(), cov) and np.array_equal(mask_d.cpu().numpy(), mask) and np.array_equal(st_d.cpu().numpy(), st)
    assert (st == 0).all() and ((mask[:, :] & 0x38) == 0x38)[wb.counts[:, 0][:, None] > np.arange(T)].all()
    # the resident batch is still there: another solve + download gives the same poses
    before = wb.poses.copy()
    s.solve_resident()
    s.download(wb)
    assert np.array_equal(wb.poses, before)


def test_one_range_per_pose_windows_are_rank_deficient(gpu):
    """The reference's own window (one anchor range per pose, zero-range smoothness edges) has 2T - 1 rank-one terms for 3T translations:
    H without the LM damping is singular (the reference's rank says so), and the relative pivot test flags every such window — the
    absolute test alone would pass the ones whose last pivots (rounding noise of either sign) come out positive."""
    import localization_amd as la
    from oracle import oracle as O
    from _covariance_ref import hessian
    rng = np.random.default_rng(31)
    B, T = 24, 10
    wb = _translation_only_batch(la, rng, B, T, False)
    s = la.WindowSolver(ANCH, B, *wb.caps, jacobian="numeric")
    s.solve(wb)
    cov, mask, st = s.covariance(wb)
    for i in range(B):
        nv = int(wb.counts[i, 0])
        assert nv > 1
        H = hessian(wb, i, ANCH, O.JAC_NUMERIC_G2O)
        keep = np.diag(H) != 0
        assert np.linalg.matrix_rank(H[np.ix_(keep, keep)]) < keep.sum()
        assert st[i] == LOC_ERR_SINGULAR and np.isnan(cov[i, :nv]).all() and not cov[i, nv:].any()


@pytest.mark.parametrize("kind", ["cfg1", "imu", "twist"])
def test_solves_are_unaffected(gpu, kind):
    """A handle that computes covariances between its solves returns the same bits (poses, results, kernel kind) as one that never does."""
    import localization_amd as la
    rng = np.random.default_rng(8)
    B, T = 32, 12
    if kind == "cfg1":
        wb = _translation_only_batch(la, rng, B, T, False)
    elif kind == "imu":
        wb = _chain_batch(la, rng, B, T, True, True)
    else:
        wb = _twist_batch(la, rng, B, T, True)
    a, b = la.WindowSolver(ANCH, B, *wb.caps), la.WindowSolver(ANCH, B, *wb.caps)
    wa, wb2 = wb.copy(), wb.copy()
    for rep in range(3):
        ra = a.solve(wa).copy()
        a.covariance(wa)
        rb = b.solve(wb2).copy()
        assert np.array_equal(wa.poses, wb2.poses) and np.array_equal(ra, rb)
        assert a.last_kernel_kind() == b.last_kernel_kind()
        wa.poses[:, :, 9:] += 0.01; wb2.poses[:, :, 9:] += 0.01


def test_covariance_leaves_the_handles_endpoint1_lever_arms_alone(gpu):
    """covariance() never changes the handle: after an upload with endpoint-1 lever arms, a refused covariance call of another batch
    leaves the resident solve exactly what it is on a handle that never made the call."""
    import localization_amd as la
    rng = np.random.default_rng(41)
    B, T = 8, 10
    wb = _translation_only_batch(la, rng, B, T, False)
    wb.r_off1 = np.zeros((B, wb.caps[1], 3)); wb.r_off1[:, :, 2] = 0.2
    a, b = la.WindowSolver(ANCH, B, *wb.caps), la.WindowSolver(ANCH, B, *wb.caps)
    wa, wc = wb.copy(), wb.copy()
    a.upload(wa); b.upload(wc)
    plain = wb.copy(); plain.r_off1 = None   # the same windows without lever arms on endpoint 1: the call reaches the library
    with pytest.raises(la.LocalizationAmdError) as ex:
        a.covariance(plain)
    assert ex.value.code == LOC_ERR_UNSUPPORTED
    a.solve_resident(); b.solve_resident()
    ra, rb = a.download(wa).copy(), b.download(wc).copy()
    assert np.array_equal(wa.poses, wc.poses) and np.array_equal(ra, rb)
