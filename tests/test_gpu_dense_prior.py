"""GPU checks of EdgeSE3Prior factors with a FULL 6 x 6 information matrix (loc_window_set_prior_information, WindowBatch.p_info): the
general window kernel against the CPU oracle with the same matrices, and the envelope covariance pass against the numpy reference of
tests/_dense_prior_ref.py.  Tolerances: DESIGN.md §3's rows of the general kernel (analytic 1e-7 m max / 1e-9 m median, numeric 1e-5 m /
1e-7 m, chi2 relative 1e-6) and tests/test_gpu_general_covariance.py's limits with its kappa rule.

Every prior of the parity cases carries a random symmetric positive-definite matrix with translation-rotation coupling: W = S C S with C a
random correlation matrix and S the scales of a 5 cm position / an IMU attitude prior."""
import functools

import numpy as np
import pytest

import _dense_prior_ref as D
import _general_cov_inputs as G
from test_gpu_general_covariance import TOL as COV_TOL
from test_gpu_snapshot_covariance import KAPPA_EPS

pytestmark = pytest.mark.gpu

ANCH = G.ANCH
LOC_ERR_INVALID, LOC_ERR_UNSUPPORTED = -1, -5
SOLVE_TOL = {"analytic": (1e-7, 1e-9), "numeric": (1e-5, 1e-7)}   # max, median [m]
SCALES = np.sqrt(np.array([400.0, 400.0, 400.0, 2e5, 2e5, 2e5]))


def _spd(rng):
    A = rng.normal(size=(6, 6))
    C = A @ A.T + 3 * np.eye(6)
    s = 1 / np.sqrt(np.diag(C))
    C = C * s[:, None] * s[None, :]
    W = SCALES[:, None] * C * SCALES[None, :]
    return 0.5 * (W + W.T)


def _densify(wb, rng, position_priors=True):
    """every prior of wb gets a full matrix (and a measurement of its own position: the IMU priors of tests/_general_cov_inputs.py hold the
    estimate); p_val's diagonal is poisoned: with the table set it is not read"""
    wb.p_info = np.zeros((wb.B, max(wb.caps[2], 1), 36))
    for i in range(wb.B):
        for e in range(int(wb.counts[i, 2])):
            wb.p_info[i, e] = _spd(rng).reshape(36)
            if position_priors:
                Ri = wb.p_val[i, e, :9].reshape(3, 3)
                wb.p_val[i, e, 9:12] -= Ri @ rng.normal(0, 0.03, 3)
            wb.p_val[i, e, 12:] = np.nan
    return wb


def _chains(la, seed, B, T, nv_max=None, two_priors=False):
    """6-DoF chains of T poses (lever arm, four anchors and a prior per pose), every prior with a full matrix"""
    nv_max = T if nv_max is None else nv_max
    wb = la.WindowBatch(B, nv_max, 5 * nv_max, nv_max + 1, 0)
    rng = np.random.default_rng(seed)
    for i in range(B):
        G.fill_chain(wb, i, rng, T, True)
        if two_priors:   # a second prior on pose T // 2
            R, t = wb.pose(i, T // 2)
            wb.add_prior(i, T // 2, t + rng.normal(0, 0.05, 3), R, np.ones(6))
    return _densify(wb, rng)


def _keyframe300(la):
    """the 300-pose key-frame window of tests/test_gpu_general_covariance.py with a full-information prior on every key frame"""
    T, every, B = 300, 10, 2
    wb = la.WindowBatch(B, T, T + 3 * (T // every + 1), T // every, T + T // every)
    rng = np.random.default_rng(9404)
    for i in range(B):
        G.fill_stars(wb, i, np.random.default_rng(9204 + i), T, every, False)
        for key in range(every - 1, T, every):
            R, t = wb.pose(i, key)
            wb.add_prior(i, key, t + rng.normal(0, 0.05, 3), R, np.ones(6))
    return _densify(wb, rng, position_priors=False)


CASES = {
    "chain1": lambda la: _chains(la, 9401, 8, 1),
    "chain2": lambda la: _chains(la, 9402, 8, 2),
    "chain12": lambda la: _chains(la, 9403, 8, 12),
    "two_priors": lambda la: _chains(la, 9405, 8, 6, two_priors=True),
    "chain70": lambda la: _chains(la, 9406, 8, 70),          # 70 pose slots: eight waves per window, arrays in the HBM workspace
    "keyframe300": _keyframe300,                              # the HBM slice, value tables read in place
}


@functools.lru_cache(maxsize=None)
def _oracle(name, jac):
    """the oracle's poses and chi2 of a case (shared, never modified)"""
    import localization_amd as la
    from oracle import oracle as O
    wb = CASES[name](la)
    mode = O.JAC_ANALYTIC if jac == "analytic" else O.JAC_NUMERIC_G2O
    out = [D.oracle_window(wb, i, ANCH, 10, mode) for i in range(wb.B)]
    return [o[0] for o in out], np.array([o[1] for o in out])


def _compare(wb, res, want, want_chi, jac, label):
    dt = np.concatenate([np.abs(wb.poses[i, :len(w), 9:] - w[:, 9:]).ravel() for i, w in enumerate(want)])
    dR = np.concatenate([np.abs(wb.poses[i, :len(w), :9] - w[:, :9]).ravel() for i, w in enumerate(want)])
    chi = np.abs(res[:, 0] - want_chi).max() / max(1.0, np.abs(want_chi).max())
    print(f"dense priors {label} {jac}: |gpu - oracle| max {dt.max():.3e} m, median {np.median(dt):.3e} m, rotation entries {dR.max():.3e}, chi2 relative {chi:.3e}")
    tol_max, tol_med = SOLVE_TOL[jac]
    assert np.isfinite(wb.poses).all()
    assert dt.max() < tol_max and np.median(dt) < tol_med and dR.max() < tol_max, (dt.max(), np.median(dt), dR.max())
    assert chi <= 1e-6, chi


@pytest.mark.parametrize("jac", ["analytic", "numeric"])
@pytest.mark.parametrize("name", list(CASES))
def test_solver_matches_the_oracle(gpu, name, jac):
    import localization_amd as la
    wb = CASES[name](la)
    want, want_chi = _oracle(name, jac)
    s = la.WindowSolver(ANCH, wb.B, *wb.caps, jacobian=jac)
    res = s.solve(wb)
    assert s.last_kernel_kind() == "window_lm_kernel"
    s.close()
    _compare(wb, res, want, want_chi, jac, name)


def test_elimination_order_is_transparent(gpu):
    """the minimum-degree order and the caller's: the table's rows go by the prior's index, whatever the labels of the poses"""
    import localization_amd as la
    want, want_chi = _oracle("chain12", "analytic")
    out = {}
    for natural in (False, True):
        wb = CASES["chain12"](la)
        s = la.WindowSolver(ANCH, wb.B, *wb.caps, jacobian="analytic", natural_order=natural)
        res = s.solve(wb)
        s.close()
        _compare(wb, res, want, want_chi, "analytic", f"chain12 natural_order={natural}")
        out[natural] = wb.poses.copy()
    assert np.abs(out[True] - out[False]).max() < 1e-7


def test_kernel_choice_diagonal_table_and_back(gpu):
    """A batch that is wave6_lm_kernel's without the table takes the general kernel with it; a table holding diag(p_val's diagonal) solves what
    the diagonals solve (to 1e-9 m: another kernel, another order of operations); NULL restores the structured kernel and its bits."""
    import localization_amd as la
    base = G.chain_batch(la, 9410, 8, 12, True, ragged=False)
    s = la.WindowSolver(ANCH, base.B, *base.caps, jacobian="analytic")
    first = base.copy()
    s.solve(first)
    assert s.last_kernel_kind() == "wave6_lm_kernel"
    diag = base.copy()
    diag.p_info = np.zeros((base.B, base.caps[2], 36))
    diag.p_info[:, :, ::7] = base.p_val[:, :, 12:]
    s.solve(diag)
    assert s.last_kernel_kind() == "window_lm_kernel"
    d = np.abs(diag.poses - first.poses).max()
    print(f"diag(p_val) as a table against the diagonals: {d:.3e}")
    assert d < 1e-9
    again = base.copy()
    s.solve(again)   # (p_info None: the harness passes NULL)
    assert s.last_kernel_kind() == "wave6_lm_kernel"
    assert np.array_equal(again.poses, first.poses) and np.array_equal(again.result, first.result)
    s.close()


def test_resident_solve_reads_the_table(gpu):
    import localization_amd as la
    wb = CASES["chain12"](la)
    host = wb.copy()
    s = la.WindowSolver(ANCH, wb.B, *wb.caps, jacobian="analytic")
    s.solve(host)
    s.upload(wb)
    s.solve_resident()
    s.download(wb)
    s.close()
    assert np.array_equal(wb.poses, host.poses) and np.array_equal(wb.result[:, :6], host.result[:, :6])


def test_refusals_change_nothing(gpu):
    import ctypes as C
    import localization_amd as la
    wb = CASES["chain12"](la)
    s = la.WindowSolver(ANCH, wb.B, *wb.caps, jacobian="analytic")
    good = wb.copy()
    s.solve(good)
    dp = C.POINTER(C.c_double)
    bad = wb.p_info.copy()
    bad[5, 3, 1 * 6 + 4] += 1e-9   # one entry of one matrix: no longer exactly symmetric
    for n, table in ((wb.B, bad), (0, wb.p_info), (-1, wb.p_info), (wb.B + 1, np.zeros((wb.B + 1, wb.caps[2], 36)))):
        assert s.L.loc_window_set_prior_information(s.h, n, np.ascontiguousarray(table).ctypes.data_as(dp)) == LOC_ERR_INVALID
    nan = wb.p_info.copy(); nan[0, 0, 1 * 6 + 2] = nan[0, 0, 2 * 6 + 1] = np.nan   # (an off-diagonal NaN on both sides: NaN != NaN)
    assert s.L.loc_window_set_prior_information(s.h, wb.B, nan.ctypes.data_as(dp)) == LOC_ERR_INVALID
    # the handle still holds the table of the last good call: the same bits
    ip = C.POINTER(C.c_int32)
    again = wb.copy()
    la._lib.check(s.L.loc_window_solve_host(s.h, again.B, again.counts.ctypes.data_as(ip), again.poses.ctypes.data_as(dp), again.r_idx.ctypes.data_as(ip),
                                            again.r_val.ctypes.data_as(dp), again.p_idx.ctypes.data_as(ip), again.p_val.ctypes.data_as(dp),
                                            again.s_idx.ctypes.data_as(ip), again.s_val.ctypes.data_as(dp), again.result.ctypes.data_as(dp)))
    assert np.array_equal(again.poses, good.poses)
    # a table of four instances: a batch of eight is refused, by the solve, the upload and the covariance call alike, and nothing is written
    assert s.L.loc_window_set_prior_information(s.h, 4, wb.p_info.ctypes.data_as(dp)) == 0
    s.set_option("covariance_general", 1)
    before = wb.poses.copy()
    args = (wb.counts.ctypes.data_as(ip), wb.poses.ctypes.data_as(dp), wb.r_idx.ctypes.data_as(ip), wb.r_val.ctypes.data_as(dp), wb.p_idx.ctypes.data_as(ip),
            wb.p_val.ctypes.data_as(dp), wb.s_idx.ctypes.data_as(ip), wb.s_val.ctypes.data_as(dp))
    cov = np.full((wb.B, wb.caps[0], 36), 7.0); mask = np.full((wb.B, wb.caps[0]), 7, dtype=np.int32); status = np.full(wb.B, 7, dtype=np.int32)
    assert s.L.loc_window_solve_host(s.h, wb.B, *args, wb.result.ctypes.data_as(dp)) == LOC_ERR_INVALID
    assert s.L.loc_window_upload(s.h, wb.B, *args) == LOC_ERR_INVALID
    assert s.L.loc_window_covariance_host(s.h, wb.B, *args, cov.ctypes.data_as(dp), mask.ctypes.data_as(ip), status.ctypes.data_as(ip)) == LOC_ERR_INVALID
    assert np.array_equal(wb.poses, before) and (cov == 7.0).all() and (mask == 7).all() and (status == 7).all()
    assert s.L.loc_window_solve_host(s.h, 4, *args, wb.result.ctypes.data_as(dp)) == 0
    assert np.array_equal(wb.poses[:4], good.poses[:4])
    s.close()
    # a solver without priors has no table to set
    s0 = la.WindowSolver(ANCH, 2, 4, 8, 0, 0)
    assert s0.L.loc_window_set_prior_information(s0.h, 2, np.zeros((2, 1, 36)).ctypes.data_as(dp)) == LOC_ERR_INVALID
    s0.close()


# ---- covariances: the envelope pass with full-information priors -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _solved(name, jac):
    import localization_amd as la
    wb = CASES[name](la)
    s = la.WindowSolver(ANCH, wb.B, *wb.caps, jacobian=jac)
    s.solve(wb)
    s.set_option("covariance_general", 1)
    out = s.covariance(wb)
    s.close()
    return wb, out


@pytest.mark.parametrize("jac", ["analytic", "numeric"])
@pytest.mark.parametrize("name", ["chain2", "chain12", "two_priors", "chain70"])
def test_covariance_matches_the_reference(gpu, name, jac):
    from oracle import oracle as O
    wb, (cov, mask, status) = _solved(name, jac)
    mode = O.JAC_ANALYTIC if jac == "analytic" else O.JAC_NUMERIC_G2O
    worst = 0.0
    for i in range(wb.B):
        nv = int(wb.counts[i, 0])
        assert status[i] == 0 and not mask[i].any() and not cov[i, nv:].any()
        want, want_mask, H = D.covariance_ref(wb, i, ANCH, mode)
        assert not want_mask.any()
        kappa = np.linalg.cond(H)
        tol = max(COV_TOL[jac], KAPPA_EPS * kappa)
        errs = [np.linalg.norm(cov[i, v] - want[v]) / np.linalg.norm(want[v]) for v in range(nv)]
        for v in range(nv):
            assert np.array_equal(cov[i, v], cov[i, v].T)
            ev = np.linalg.eigvalsh(cov[i, v])
            assert ev.min() >= -1e-12 * ev.max()
        print(f"dense-prior covariance {name} {jac} window {i}: max relative Frobenius error {max(errs):.3e}, kappa {kappa:.3e}, limit {tol:.3e}")
        worst = max(worst, max(errs))
        assert max(errs) <= tol, (i, max(errs), tol, kappa)
    print(f"dense-prior covariance {name} {jac}: max relative Frobenius error {worst:.3e}")


def test_covariance_needs_the_general_option_and_joint_calls_follow(gpu):
    import localization_amd as la
    from localization_amd._lib import LocalizationAmdError
    from oracle import oracle as O
    wb, (cov, mask, status) = _solved("chain12", "analytic")
    wb = wb.copy()
    s = la.WindowSolver(ANCH, wb.B, *wb.caps, jacobian="analytic")
    out = (np.full((wb.B, wb.caps[0], 6, 6), 7.0), np.full((wb.B, wb.caps[0]), 7, dtype=np.int32), np.full(wb.B, 7, dtype=np.int32))
    with pytest.raises(LocalizationAmdError) as e:   # a chain batch of twelve poses: covariance_kernel<6>'s — but that pass reads the diagonals
        s.covariance(wb, out=out)
    assert e.value.code == LOC_ERR_UNSUPPORTED
    assert (out[0] == 7.0).all() and (out[1] == 7).all() and (out[2] == 7).all()
    jout = out + (np.full((wb.B, 2, 6, 6), 7.0),)
    pairs = np.array([[0, 1], [3, 11]])
    with pytest.raises(LocalizationAmdError) as e:
        s.joint_covariance(wb, pairs, out=jout)
    assert e.value.code == LOC_ERR_UNSUPPORTED and (jout[3] == 7.0).all() and (jout[0] == 7.0).all()
    s.set_option("covariance_general", 1)
    c2, m2, s2, cross = s.joint_covariance(wb, pairs)
    assert np.array_equal(c2, cov) and np.array_equal(m2, mask) and np.array_equal(s2, status)
    for i in range(wb.B):
        H = D.hessian(wb, i, ANCH, O.JAC_ANALYTIC)
        Sig = np.linalg.inv(H)
        for p, (a, b) in enumerate(pairs):
            want = Sig[6 * a:6 * a + 6, 6 * b:6 * b + 6]
            scale = np.sqrt(np.linalg.norm(Sig[6 * a:6 * a + 6, 6 * a:6 * a + 6]) * np.linalg.norm(Sig[6 * b:6 * b + 6, 6 * b:6 * b + 6]))
            assert np.linalg.norm(cross[i, p] - want) <= max(COV_TOL["analytic"], KAPPA_EPS * np.linalg.cond(H)) * scale
    # the resident batch: classified as a chain by the upload, served by the envelope pass while the table is set
    import torch
    s.upload(wb)
    s.solve_resident()
    dev = torch.device("cuda", 0)
    tc = torch.zeros((wb.B, wb.caps[0], 36), dtype=torch.float64, device=dev)
    tm = torch.zeros((wb.B, wb.caps[0]), dtype=torch.int32, device=dev); ts = torch.zeros(wb.B, dtype=torch.int32, device=dev)
    s.covariance_resident(tc, tm, ts)
    torch.cuda.synchronize()
    res = la.WindowBatch(wb.B, *wb.caps)
    s.download(res)
    host = wb.copy(); host.poses[:] = res.poses
    want = s.covariance(host)
    assert np.array_equal(tc.cpu().numpy().reshape(want[0].shape), want[0]) and not ts.cpu().numpy().any()
    s.close()
