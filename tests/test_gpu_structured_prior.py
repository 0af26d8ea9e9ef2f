"""GPU checks of option "prior_information_structured": a translation-only table of full information matrices (dense 3 x 3 blocks on the
translations — what loc_window_marginal_prior_host hands out) on translation-only chains of <= 64 poses is solved by
wave3_lm_kernel<JAC, true> and served by the chain 3 x 3 covariance pass covariance_kernel<3, .., true>.

Inputs: tests/_structured_prior_cases.py (eight windows per case; regular by the reference alone: tests/test_structured_prior_cpu.py) and the
fixed-lag chains of tests/_fixed_lag.py.  References: the CPU oracle with the same matrices (tests/_dense_prior_ref.oracle_window) for the
solves, tests/_dense_prior_ref.covariance_ref / marginal_ref at the GPU's poses for covariances and marginals.

Tolerances: solves — analytic 1e-7 m max / 1e-9 m median, numeric 1e-5 m / 1e-7 m, chi2 relative 1e-6; one kernel against
another on the same inputs — 1e-9 m (tests/test_gpu_dense_prior.py::test_kernel_choice_diagonal_table_and_back); covariances — the chain
file's (tests/test_gpu_covariance.py: analytic 1e-8, numeric 1.5e-9), per window max(limit, 1e-15 kappa(H_kept)); the envelope pass
against the chain pass — the envelope file's max(8.4e-12, 1e-15 kappa)."""
import ctypes as C
import functools

import numpy as np
import pytest

import _dense_prior_ref as D
import _fixed_lag as F
import _structured_prior_cases as S
from test_gpu_covariance import TOL as COV_TOL
from test_gpu_general_covariance import TOL as ENVELOPE_TOL
from test_gpu_marginal_prior import _check_window as _check_marginal
from test_gpu_snapshot_covariance import KAPPA_EPS

pytestmark = pytest.mark.gpu

LOC_ERR_INVALID, LOC_ERR_UNSUPPORTED, LOC_ERR_SINGULAR = -1, -5, -6
SOLVE_TOL = {"analytic": (1e-7, 1e-9), "numeric": (1e-5, 1e-7)}   # max, median [m]
KERNEL_TOL = 1e-9                                                  # another kernel, another order of operations [m]
ANCH = S.ANCH
OPTION = "prior_information_structured"


def _mode(O, jac):
    return O.JAC_ANALYTIC if jac == "analytic" else O.JAC_NUMERIC_G2O


def _solver(la, wb, jac, structured=1, **kw):
    s = la.WindowSolver(ANCH, wb.B, *wb.caps, jacobian=jac, **kw)
    s.set_option(OPTION, structured)
    return s


def _oracle_of(wb, jac):
    from oracle import oracle as O
    out = [D.oracle_window(wb, i, ANCH, 10, _mode(O, jac)) for i in range(wb.B)]
    return [o[0] for o in out], np.array([o[1] for o in out])


@functools.lru_cache(maxsize=None)
def _oracle(name, jac):
    """the oracle's poses and chi2 of a case (shared, never modified)"""
    import localization_amd as la
    return _oracle_of(S.case_batch(la, name), jac)


def _compare(wb, res, want, want_chi, jac, label):
    dt = np.concatenate([np.abs(wb.poses[i, :len(w), 9:] - w[:, 9:]).ravel() for i, w in enumerate(want)])
    dR = np.concatenate([np.abs(wb.poses[i, :len(w), :9] - w[:, :9]).ravel() for i, w in enumerate(want)])
    chi = np.abs(res[:, 0] - want_chi).max() / max(1.0, np.abs(want_chi).max())
    print(f"structured priors {label} {jac}: |gpu - oracle| max {dt.max():.3e} m, median {np.median(dt):.3e} m, rotation entries {dR.max():.3e}, chi2 relative {chi:.3e}")
    tol_max, tol_med = SOLVE_TOL[jac]
    assert np.isfinite(wb.poses).all()
    assert dt.max() < tol_max and np.median(dt) < tol_med and dR.max() < tol_max, (dt.max(), np.median(dt), dR.max())
    assert chi <= 1e-6, chi


@functools.lru_cache(maxsize=None)
def _solved(name, jac):
    """(batch at the GPU's poses, result, kernel) of a case solved with the option on; shared, never modified"""
    import localization_amd as la
    wb = S.case_batch(la, name)
    s = _solver(la, wb, jac)
    res = s.solve(wb).copy()
    kind = s.last_kernel_kind()
    s.close()
    return wb, res, kind


# ---- 1. parity with the oracle ---------------------------------------------------------------------------------------------------------------
PARITY = [n for n in S.CASES if n != "singular"]


@pytest.mark.parametrize("jac", ["analytic", "numeric"])
@pytest.mark.parametrize("name", PARITY)
def test_solver_matches_the_oracle(gpu, name, jac):
    wb, res, kind = _solved(name, jac)
    assert kind == "wave3_lm_kernel"
    want, want_chi = _oracle(name, jac)
    _compare(wb, res, want, want_chi, jac, name)


# ---- 2. the twin against the general kernel's twin ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["T6", "T10", "T40x2", "doubled", "zprior"])
def test_twin_against_the_general_kernel_and_back(gpu, name):
    import localization_amd as la
    base = S.case_batch(la, name)
    s = _solver(la, base, "analytic", structured=0)
    general = base.copy()
    s.solve(general)
    assert s.last_kernel_kind() == "window_lm_kernel"
    s.set_option(OPTION, 1)
    twin = base.copy()
    s.solve(twin)
    assert s.last_kernel_kind() == "wave3_lm_kernel"
    d = np.abs(twin.poses - general.poses).max()
    print(f"wave3_lm_kernel<0, true> against window_lm_kernel<.., PINFO> {name}: {d:.3e} m")
    assert d <= KERNEL_TOL
    s.set_option(OPTION, 0)
    again = base.copy()
    s.solve(again)
    assert s.last_kernel_kind() == "window_lm_kernel"
    assert np.array_equal(again.poses, general.poses) and np.array_equal(again.result, general.result)
    s.close()


def test_option_values(gpu):
    import localization_amd as la
    from localization_amd._lib import LocalizationAmdError
    s = la.WindowSolver(ANCH, 2, *S.caps(6, 1))
    for bad in (-1, 2, 7):
        with pytest.raises(LocalizationAmdError) as e:
            s.set_option(OPTION, bad)
        assert e.value.code == LOC_ERR_INVALID
    s.set_option(OPTION, 1); s.set_option(OPTION, 0)
    s.close()


# ---- 3. a table holding the diagonals against no table: wave3_lm_kernel<JAC, true> against <JAC, false> -------------------------------------------
@pytest.mark.parametrize("jac", ["analytic", "numeric"])
def test_diagonal_table_against_the_diagonals_and_back(gpu, jac):
    import localization_amd as la
    base = S.diagonal_batch(la)
    s = _solver(la, base, jac)
    first = base.copy()
    s.solve(first)
    assert s.last_kernel_kind() == "wave3_lm_kernel"
    diag = base.copy()
    diag.p_info = np.zeros((base.B, base.caps[2], 36))
    diag.p_info[:, :, ::7] = base.p_val[:, :, 12:]
    s.solve(diag)
    assert s.last_kernel_kind() == "wave3_lm_kernel"
    d = np.abs(diag.poses - first.poses).max()
    print(f"diag(p_val) as a structured table against the diagonals {jac}: {d:.3e} m, same bits: {np.array_equal(diag.poses, first.poses) and np.array_equal(diag.result, first.result)}")
    assert d <= KERNEL_TOL
    again = base.copy()
    s.solve(again)   # (p_info None: the harness passes NULL)
    assert s.last_kernel_kind() == "wave3_lm_kernel"
    assert np.array_equal(again.poses, first.poses) and np.array_equal(again.result, first.result)
    s.close()


# ---- 4. fall-backs ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["rotation_entry", "rotated_pose", "wave3_off", "natural_order"])
def test_fall_backs_take_the_general_kernel(gpu, how):
    import localization_amd as la
    wb = S.case_batch(la, "T6")
    kw = {"natural_order": True} if how == "natural_order" else {}
    if how == "rotation_entry":
        wb.p_info[2, 0, 4 * 6 + 4] = 25.0
    if how == "rotated_pose":
        c, sn = np.cos(0.1), np.sin(0.1)
        wb.poses[5, 2, :9] = (c, -sn, 0, sn, c, 0, 0, 0, 1)
    want, want_chi = _oracle("T6", "analytic") if how in ("wave3_off", "natural_order") else _oracle_of(wb, "analytic")
    s = _solver(la, wb, "analytic", **kw)
    if how == "wave3_off":
        s.set_option("wave3", 0)
    res = s.solve(wb)
    assert s.last_kernel_kind() == "window_lm_kernel"
    s.close()
    _compare(wb, res, want, want_chi, "analytic", f"fall-back {how}")


# ---- 5. the resident path ----------------------------------------------------------------------------------------------------------------------------
def _with_rotation_diagonals(la):
    """T6 with p_val's diagonals filled in: the table's own translation diagonal, and ROTATION information — without the table the batch is a
    6-DoF chain"""
    wb = S.case_batch(la, "T6")
    wb.p_val[:, :, 12:15] = wb.p_info[:, :, [0, 7, 14]]
    wb.p_val[:, :, 15:18] = 50.0
    return wb


def _download(la, s, like):
    out = la.WindowBatch(like.B, *like.caps)
    s.download(out)
    return out


def _used(wb):
    return np.arange(wb.caps[0])[None, :] < wb.counts[:, :1]


def test_resident_solve_has_the_host_solves_bits(gpu):
    import torch
    import localization_amd as la
    base = _with_rotation_diagonals(la)
    s = _solver(la, base, "numeric")
    host = base.copy()
    s.solve(host)
    assert s.last_kernel_kind() == "wave3_lm_kernel"
    s.upload(base)
    for stream in (None, torch.cuda.Stream()):
        s.solve_resident(None if stream is None else C.c_void_p(stream.cuda_stream))
        assert s.last_kernel_kind() == "wave3_lm_kernel"
        res = _download(la, s, base)
        assert np.array_equal(res.poses[_used(base)], host.poses[_used(base)]) and np.array_equal(res.result[:, :6], host.result[:, :6])
    s.close()


@pytest.mark.parametrize("change", ["table_null", "option_off", "rotation_table"])
def test_resident_verdict_does_not_outlive_the_structured_table(gpu, change):
    """The upload's verdict was taken with the priors' diagonals skipped.  Once the table has gone (the diagonals count again — and hold rotation
    information here), has got a rotation entry, or the option is off, the resident solve must not reach wave3_lm_kernel."""
    import localization_amd as la
    base = _with_rotation_diagonals(la)
    s = _solver(la, base, "analytic")
    s.upload(base)
    s.solve_resident()
    assert s.last_kernel_kind() == "wave3_lm_kernel"
    now = base.copy()   # the batch a host call would be given now
    dp = C.POINTER(C.c_double)
    if change == "table_null":
        assert s.L.loc_window_set_prior_information(s.h, 0, None) == 0
        now.p_info = None
    elif change == "option_off":
        s.set_option(OPTION, 0)
    else:
        now.p_info[:, :, 3 * 6 + 3] = 40.0
        assert s.L.loc_window_set_prior_information(s.h, now.B, now.p_info.ctypes.data_as(dp)) == 0
    s.solve_resident()
    kind = s.last_kernel_kind()
    res = _download(la, s, base)
    s.solve(now)
    print(f"resident solve after {change}: {kind}; the host call takes {s.last_kernel_kind()}")
    assert kind == "window_lm_kernel" and s.last_kernel_kind() != "wave3_lm_kernel"
    s.close()
    dt = np.abs(res.poses[_used(base)] - now.poses[_used(base)])
    print(f"resident solve after {change} against the host solve: max {dt.max():.3e}, median {np.median(dt):.3e}")
    assert dt.max() < SOLVE_TOL["analytic"][0] and np.median(dt) < SOLVE_TOL["analytic"][1]


# ---- 6. the fixed-lag chain end to end ------------------------------------------------------------------------------------------------------------------
W, SLIDES = 6, 3


@pytest.mark.parametrize("jac", ["analytic", "numeric"])
def test_fixed_lag_chain_on_the_wave_kernel(gpu, jac):
    """tests/test_gpu_marginal_prior.py::test_fixed_lag_chain_against_the_oracle_chain with the option on: every window after the first slide
    carries a full-information prior and is solved by wave3_lm_kernel"""
    import localization_amd as la
    from oracle import oracle as O
    mode = _mode(O, jac)
    chains = [F.Chain(7900 + i, W + SLIDES, 3 + i % 2) for i in range(8)]
    s = la.WindowSolver(ANCH, len(chains), *F.window_caps(W), jacobian=jac)
    s.set_option(OPTION, 1)
    g = F.first_window(la, chains, W)
    tol_max, tol_med = SOLVE_TOL[jac]
    for k in range(SLIDES + 1):
        o = g.copy()
        res = s.solve(g)
        assert s.last_kernel_kind() == "wave3_lm_kernel", (k, s.last_kernel_kind())
        want_chi = np.zeros(o.B)
        for i in range(o.B):
            o.poses[i, :W], want_chi[i], _ = D.oracle_window(o, i, ANCH, 10, mode)
        dt = np.abs(g.poses[:, :, 9:] - o.poses[:, :, 9:])
        chi = np.abs(res[:, 0] - want_chi).max() / max(1.0, np.abs(want_chi).max())
        print(f"fixed lag (structured) {jac} window {k}: |gpu - oracle| max {dt.max():.3e} m, median {np.median(dt):.3e} m, chi2 relative {chi:.3e}")
        assert dt.max() < tol_max and np.median(dt) < tol_med and chi <= 1e-6, (k, dt.max(), np.median(dt), chi)
        if k == SLIDES:
            break
        out = s.marginal_prior(g, 0)
        slot, prior, status = out[0], out[1], out[5]
        assert not status.any() and (slot == 1).all()
        for i in range(g.B):
            assert _check_marginal(g, i, 0, D.marginal_ref(g, i, ANCH, mode, 0), out, jac, f"fixed lag (structured) slide {k + 1}") is not None
        g = F.next_window(la, g, chains, k + 1, W, slot, prior)
    s.close()


# ---- 7. covariances ----------------------------------------------------------------------------------------------------------------------------------------
def _pairs(T):
    return np.array([[0, T - 1], [T - 1, 0], [T // 2, T // 2], [min(1, T - 1), 0]], dtype=np.int32)


PAIR_COUNTS = np.array([4, 3, 4, 2, 0, 4, 1, 4], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def _covariances(name, jac):
    """a covariance case at the GPU's poses: the host call, the joint host call; shared, never modified"""
    import localization_amd as la
    wb, _, _ = _solved(name, jac)
    s = _solver(la, wb, jac)
    plain = s.covariance(wb)
    assert s.last_covariance_ms() > 0
    joint = s.joint_covariance(wb, _pairs(wb.caps[0]), PAIR_COUNTS)
    s.close()
    return wb, plain, joint


def _check_cov(O, wb, jac, cov, mask, status, label, skip=()):
    mode = _mode(O, jac)
    worst, relaxed = 0.0, False
    for i in range(wb.B):
        nv = int(wb.counts[i, 0])
        if i in skip:
            continue
        assert status[i] == 0, (i, status[i])
        assert not cov[i, nv:].any() and not mask[i, nv:].any()
        assert (mask[i, :nv] == 0b111000).all(), (i, mask[i, :nv])
        assert not cov[i, :, 3:, :].any() and not cov[i, :, :, 3:].any()
        want, want_mask, H = D.covariance_ref(wb, i, ANCH, mode)
        assert np.array_equal(mask[i, :nv], want_mask)
        keep = np.diag(H) != 0
        kappa = np.linalg.cond(H[np.ix_(keep, keep)])
        tol = max(COV_TOL[jac], KAPPA_EPS * kappa)
        relaxed = relaxed or tol > COV_TOL[jac]
        errs = []
        for v in range(nv):
            g, r = cov[i, v], want[v]
            errs.append(np.linalg.norm(g - r) / np.linalg.norm(r))
            assert np.array_equal(g, g.T)
            ev = np.linalg.eigvalsh(g)
            assert ev.min() >= -1e-12 * ev.max()
        worst = max(worst, max(errs))
        assert max(errs) <= tol, (label, i, max(errs), tol, kappa)
    print(f"structured-prior covariance {label} {jac}: max relative Frobenius error {worst:.3e}, kappa rule applied: {relaxed}")
    return worst


@pytest.mark.parametrize("jac", ["analytic", "numeric"])
@pytest.mark.parametrize("name", S.COV_CASES)
def test_covariance_matches_the_reference(gpu, name, jac):
    from oracle import oracle as O
    wb, (cov, mask, status), (jc, jm, js, cross) = _covariances(name, jac)
    _check_cov(O, wb, jac, cov, mask, status, name)
    # the joint call: the same diagonal blocks, and the cross blocks against the dense inverse
    assert np.array_equal(jc, cov) and np.array_equal(jm, mask) and np.array_equal(js, status)
    pairs = _pairs(wb.caps[0])
    mode = _mode(O, jac)
    worst = 0.0
    for i in range(wb.B):
        H = D.hessian(wb, i, ANCH, mode)
        keep = np.diag(H) != 0
        Sig = np.zeros_like(H)
        Sig[np.ix_(keep, keep)] = np.linalg.inv(H[np.ix_(keep, keep)])
        tol = max(COV_TOL[jac], KAPPA_EPS * np.linalg.cond(H[np.ix_(keep, keep)]))
        assert not cross[i, PAIR_COUNTS[i]:].any()
        for p in range(PAIR_COUNTS[i]):
            a, b = pairs[p]
            want = Sig[6 * a:6 * a + 6, 6 * b:6 * b + 6]
            scale = np.sqrt(np.linalg.norm(Sig[6 * a:6 * a + 6, 6 * a:6 * a + 6]) * np.linalg.norm(Sig[6 * b:6 * b + 6, 6 * b:6 * b + 6]))
            e = np.linalg.norm(cross[i, p] - want) / scale
            worst = max(worst, e)
            assert e <= tol, (i, p, e, tol)
        if PAIR_COUNTS[i] >= 2:
            assert np.array_equal(cross[i, 1], cross[i, 0].T)                       # (j, i) is the transpose of (i, j), bit for bit
        if PAIR_COUNTS[i] >= 3:
            assert np.array_equal(cross[i, 2], cov[i, wb.caps[0] // 2])              # (i, i) has the bits of cov[i]
    print(f"structured-prior joint covariance {name} {jac}: largest cross-block error {worst:.3e}")


@pytest.mark.parametrize("name", ["T6", "T40x2"])
def test_resident_covariances_have_the_host_calls_bits(gpu, name):
    import torch
    import localization_amd as la
    base = S.case_batch(la, name)
    s = _solver(la, base, "numeric")
    s.upload(base)
    s.solve_resident()
    assert s.last_kernel_kind() == "wave3_lm_kernel"
    dev = torch.device("cuda", 0)
    nvm = base.caps[0]
    pairs = _pairs(nvm)
    tc = torch.zeros((base.B, nvm, 36), dtype=torch.float64, device=dev); tj = torch.zeros_like(tc)
    tm = torch.zeros((base.B, nvm), dtype=torch.int32, device=dev); ts = torch.zeros(base.B, dtype=torch.int32, device=dev)
    tx = torch.zeros((base.B, len(pairs), 36), dtype=torch.float64, device=dev)
    s.covariance_resident(tc, tm, ts)
    s.joint_covariance_resident(pairs, PAIR_COUNTS, tj, tm, ts, tx)
    torch.cuda.synchronize()
    host = base.copy()
    host.poses[:] = _download(la, s, base).poses
    host.poses[~_used(base)] = base.poses[~_used(base)]
    cov, mask, status, cross = s.joint_covariance(host, pairs, PAIR_COUNTS)
    s.close()
    assert not status.any()
    assert np.array_equal(tc.cpu().numpy().reshape(cov.shape), cov) and np.array_equal(tj.cpu().numpy().reshape(cov.shape), cov)
    assert np.array_equal(tm.cpu().numpy(), mask) and not ts.cpu().numpy().any()
    assert np.array_equal(tx.cpu().numpy().reshape(cross.shape), cross)


def test_covariance_without_the_option_and_the_envelope_pass(gpu):
    import localization_amd as la
    from localization_amd._lib import LocalizationAmdError
    for jac in ("analytic", "numeric"):
        wb, (cov, mask, status), _ = _covariances("T10", jac)
        wb = wb.copy()
        s = _solver(la, wb, jac, structured=0)
        out = (np.full((wb.B, wb.caps[0], 6, 6), 7.0), np.full((wb.B, wb.caps[0]), 7, dtype=np.int32), np.full(wb.B, 7, dtype=np.int32))
        with pytest.raises(LocalizationAmdError) as e:
            s.covariance(wb, out=out)
        assert e.value.code == LOC_ERR_UNSUPPORTED and (out[0] == 7.0).all() and (out[1] == 7).all() and (out[2] == 7).all()
        s.set_option("covariance_general", 1)
        ec, em, es = s.covariance(wb)
        # ... and with both options on the chain pass keeps the batch: its bits
        s.set_option(OPTION, 1)
        c2, m2, s2 = s.covariance(wb)
        s.close()
        assert np.array_equal(c2, cov) and np.array_equal(m2, mask) and np.array_equal(s2, status)
        assert np.array_equal(em, mask) and not es.any()
        worst = 0.0
        for i in range(wb.B):
            H = D.hessian(wb, i, ANCH, O_mode(jac))
            keep = np.diag(H) != 0
            tol = max(ENVELOPE_TOL[jac], KAPPA_EPS * np.linalg.cond(H[np.ix_(keep, keep)]))
            for v in range(int(wb.counts[i, 0])):
                e = np.linalg.norm(ec[i, v] - cov[i, v]) / np.linalg.norm(cov[i, v])
                worst = max(worst, e)
                assert e <= tol, (jac, i, v, e, tol)
        print(f"envelope pass against covariance_kernel<3, .., true> {jac}: max relative Frobenius difference {worst:.3e}")


def O_mode(jac):
    from oracle import oracle as O
    return _mode(O, jac)


def test_singular_window_leaves_its_neighbours_alone(gpu):
    """window 3 keeps one anchor range per pose: LOC_ERR_SINGULAR and NaN; the other windows return the bits they return in the batch where
    window 3 keeps all its ranges"""
    import localization_amd as la
    from oracle import oracle as O
    wb, _, kind = _solved("singular", "analytic")
    assert kind == "wave3_lm_kernel"
    bad = S.SINGULAR["singular"]
    others = [i for i in range(wb.B) if i not in bad]
    s = _solver(la, wb, "analytic")
    cov, mask, status, cross = s.joint_covariance(wb, _pairs(wb.caps[0]), PAIR_COUNTS)
    for i in bad:
        nv = int(wb.counts[i, 0])
        assert status[i] == LOC_ERR_SINGULAR and np.isnan(cov[i, :nv]).all() and np.isnan(cross[i, :PAIR_COUNTS[i]]).all()
    assert not status[others].any()
    _check_cov(O, wb, "analytic", cov, mask, status, "singular", skip=bad)
    saved = S.CASES["singular"]
    try:
        S.CASES["singular"] = [dict(sp, singular=False) for sp in saved]
        full = S.case_batch(la, "singular")
    finally:
        S.CASES["singular"] = saved
    full.poses[:] = wb.poses
    c2, m2, s2, x2 = s.joint_covariance(full, _pairs(wb.caps[0]), PAIR_COUNTS)
    s.close()
    assert not s2.any()
    assert np.array_equal(c2[others], cov[others]) and np.array_equal(m2[others], mask[others]) and np.array_equal(x2[others], cross[others])
