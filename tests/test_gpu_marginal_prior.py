"""GPU checks of the marginal prior of a dropped pose (marginal_prior_kernel.hip through loc_window_marginal_prior_host) against the numpy
statement of DESIGN.md §2 (tests/_dense_prior_ref.marginal_ref) at the estimates the GPU's solve returns, and of the fixed-lag smoother built
from it (tests/_fixed_lag.py) against the same chain on the oracle.  Inputs: tests/_fixed_lag.py; every input meant to pass is regular by the
reference alone (tests/test_marginal_prior_cpu.py at the oracle-solved poses).

Errors: Lambda — the output information against the reference's, ||D||_F / ||Lambda_ref||_F; gamma — relative to
|g_m| + |H_md H_dd^-1 g_d| (gamma is the difference of the two and can be near 0); e0 — relative to |e0| and to lambda_max / lambda_min,kept.
Limits: analytic the project's 1e-8; numeric 10x the largest value measured over every case of this file on an MI355X (DESIGN.md §3 lists the
cases); a window is held to max(limit, 1e-15 kappa(H^r_dd))."""
import ctypes as C
import functools

import numpy as np
import pytest

import _dense_prior_ref as D
import _fixed_lag as F

pytestmark = pytest.mark.gpu

LOC_ERR_INVALID, LOC_ERR_UNSUPPORTED, LOC_ERR_SINGULAR = -1, -5, -6
TOL = {"analytic": 1e-8, "numeric": 1.2e-12}   # numeric: 10 x 1.166e-13 (e0 of "one_range", window 0; DESIGN.md §3 lists every case)
SOLVE_TOL = {"analytic": (1e-7, 1e-9), "numeric": (1e-5, 1e-7)}   # max, median [m]: DESIGN.md §3's rows of the solve kernels
ANCH = F.ANCH
IDENTITY_ROW = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1] + [0] * 39, dtype=float)


def _mode(O, jac):
    return O.JAC_ANALYTIC if jac == "analytic" else O.JAC_NUMERIC_G2O


@functools.lru_cache(maxsize=None)
def _solved(name, jac):
    """(batch at the GPU's poses, drop, the marginal pass's six outputs) of a parity case; shared, never modified"""
    import localization_amd as la
    wb, drop = F.case_batch(la, name)
    s = la.WindowSolver(ANCH, wb.B, *wb.caps, jacobian=jac)
    s.solve(wb)
    out = s.marginal_prior(wb, drop)
    assert s.last_covariance_ms() > 0
    s.close()
    return wb, drop, out


def _check_window(wb, i, d, ref, out, jac, label):
    """every assertion on one window's row; returns its (Lambda, gamma, e0) errors, None for a window without a carried prior"""
    slot, prior, grad, shift, rank, status = (x[i] for x in out)
    assert slot == ref["slot"] and rank == ref["rank"] and status == ref["status"], (label, i, slot, rank, status, ref["slot"], ref["rank"], ref["status"])
    info = prior[12:].reshape(6, 6)
    assert np.array_equal(prior[:9], IDENTITY_ROW[:9]) and np.array_equal(info, info.T)
    assert not info[3:].any() and not info[:, 3:].any() and not grad[3:].any() and not shift[3:].any()
    if slot < 0:
        assert np.array_equal(prior, IDENTITY_ROW) and not grad.any() and not shift.any() and rank == 0 and status == 0
        return None
    Xm = wb.poses[i, slot]
    assert np.abs(D.prior_residual(prior, Xm) - shift[:3]).max() <= 1e-15
    if status == LOC_ERR_SINGULAR:   # the zero row: the plain drop
        assert not info.any() and not grad.any() and not shift.any() and rank == 0 and np.array_equal(prior[9:12], 0.0 - Xm[9:12])
        return None
    ev = np.linalg.eigvalsh(info[:3, :3])
    assert ev.min() >= -1e-15 * ev.max()
    lam = ref["eig"]
    kept = lam[lam > D.REL_PIVOT * lam.max()]
    tol = max(TOL[jac], 1e-15 * ref["kappa"])
    e_lam = np.linalg.norm(info - ref["prior"][12:].reshape(6, 6)) / np.linalg.norm(ref["Lam"])
    e_gam = np.linalg.norm(grad - ref["grad"]) / ref["term"]
    e_e0 = np.linalg.norm(shift - ref["shift"]) / np.linalg.norm(ref["shift"]) / (kept.max() / kept.min())
    print(f"marginal prior {label} {jac} window {i}: Lambda {e_lam:.3e}, gamma {e_gam:.3e}, e0 {e_e0:.3e}, rank {rank}, kappa(H_dd) {ref['kappa']:.3e}, limit {tol:.3e}")
    assert e_lam <= tol and e_gam <= tol and e_e0 <= tol, (label, i, e_lam, e_gam, e_e0, tol)
    return e_lam, e_gam, e_e0


@pytest.mark.parametrize("jac", ["analytic", "numeric"])
@pytest.mark.parametrize("name", list(F.CASES))
def test_parity_with_the_numpy_statement(gpu, name, jac):
    from oracle import oracle as O
    wb, drop, out = _solved(name, jac)
    errs = []
    for i in range(wb.B):
        ref = D.marginal_ref(wb, i, ANCH, _mode(O, jac), int(drop[i]))
        e = _check_window(wb, i, int(drop[i]), ref, out, jac, name)
        if e is not None:
            errs.append(e)
    slot, status = out[0], out[5]
    specs = F.CASES[name]
    for i, s in enumerate(specs):
        assert (slot[i] < 0) == (s["T"] == 1 or (bool(s.get("missing")) and s["drop"] in (0, 1))), (i, slot[i])
        assert (status[i] == LOC_ERR_SINGULAR) == bool(s.get("one_range"))
    if errs:
        print(f"marginal prior {name} {jac}: largest errors Lambda {max(e[0] for e in errs):.3e}, gamma {max(e[1] for e in errs):.3e}, e0 {max(e[2] for e in errs):.3e}")
    else:
        assert name == "chain1"


def test_singular_window_leaves_its_neighbours_alone(gpu):
    """the windows whose dropped pose keeps one anchor range return the zero row; the other windows of the batch return the bits they return
    in the batch where those two keep all their ranges"""
    import localization_amd as la
    wb, drop, out = _solved("one_range", "analytic")
    singular = [i for i, s in enumerate(F.CASES["one_range"]) if s.get("one_range")]
    assert singular and (out[5][singular] == LOC_ERR_SINGULAR).all() and (out[0][singular] == 1).all()
    saved = F.CASES["one_range"]
    try:
        F.CASES["one_range"] = [dict(s, one_range=False) for s in saved]
        full, _ = F.case_batch(la, "one_range")
    finally:
        F.CASES["one_range"] = saved
    others = [i for i in range(wb.B) if i not in singular]
    s = la.WindowSolver(ANCH, wb.B, *wb.caps, jacobian="analytic")
    s.solve(full)
    assert np.array_equal(full.poses[others], wb.poses[others])
    again = s.marginal_prior(full, drop)
    s.close()
    assert not again[5].any()
    for a, b in zip(out, again):
        assert np.array_equal(a[others], b[others])


@pytest.mark.parametrize("jac", ["analytic", "numeric"])
def test_same_bits_elsewhere_in_the_batch_on_a_second_run_and_through_the_large_path(gpu, jac):
    import localization_amd as la
    wb, drop, out = _solved("ragged", jac)
    s = la.WindowSolver(ANCH, 1300, *wb.caps, jacobian=jac)
    again = s.marginal_prior(wb, drop)
    order = np.array([5, 2, 7, 0, 3, 6, 1, 4])
    moved = wb.take(order)
    there = s.marginal_prior(moved, drop[order])
    # 1 296 windows: beyond the staging block, through the pass's own device block
    reps = 162
    big = wb.tile(wb.B * reps)
    large = s.marginal_prior(big, np.concatenate([drop] * reps))
    s.close()
    for a, b, c, d in zip(out, again, there, large):
        assert np.array_equal(a, b) and np.array_equal(a[order], c)
        assert np.array_equal(d.reshape((reps,) + a.shape), np.broadcast_to(a, (reps,) + a.shape))


def _poisoned(B):
    return (np.full(B, 7, dtype=np.int32), np.full((B, 48), 7.0), np.full((B, 6), 7.0), np.full((B, 6), 7.0), np.full(B, 7, dtype=np.int32), np.full(B, 7, dtype=np.int32))


def _untouched(out):
    return all((x == 7).all() for x in out)


def test_unsupported_and_invalid_calls_write_nothing(gpu):
    import localization_amd as la
    from localization_amd._lib import LocalizationAmdError
    wb, drop, _ = _solved("chain10", "analytic")
    s = la.WindowSolver(ANCH, wb.B, *wb.caps, jacobian="analytic")

    def refused(batch, d, code):
        out = _poisoned(batch.B)
        with pytest.raises(LocalizationAmdError) as e:
            s.marginal_prior(batch, d, out=out)
        assert e.value.code == code and _untouched(out), (e.value.code, code)

    for window, slot in ((0, -1), (7, 10), (3, 2 ** 31 - 1)):          # a drop slot outside the window
        d = drop.copy(); d[window] = slot
        refused(wb, d, LOC_ERR_INVALID)
    d = drop.copy(); d[5] = 4                                           # an inner pose: two neighbours
    refused(wb, d, LOC_ERR_UNSUPPORTED)
    d[2] = 10                                                           # ... and an invalid slot elsewhere is invalid first
    refused(wb, d, LOC_ERR_INVALID)
    tilted = wb.copy()                                              # not translation-only: one rotated pose
    c, sn = np.cos(0.1), np.sin(0.1)
    tilted.poses[6, 3, :9] = (c, -sn, 0, sn, c, 0, 0, 0, 1)
    refused(tilted, drop, LOC_ERR_UNSUPPORTED)
    levered = wb.copy(); levered.r_val[1, 0, 2] = 0.01              # a lever arm
    refused(levered, drop, LOC_ERR_UNSUPPORTED)
    coupled, cdrop = F.case_batch(la, "fullprior")                       # a full-information prior with a translation-rotation entry
    coupled.p_info[4, 1, 2 * 6 + 5] = coupled.p_info[4, 1, 5 * 6 + 2] = 1e-3
    refused(coupled, cdrop, LOC_ERR_UNSUPPORTED)
    # endpoint-1 lever arms set on the handle
    dp = C.POINTER(C.c_double)
    off1 = np.zeros((wb.B, wb.caps[1], 3))
    assert s.L.loc_window_set_endpoint1_offsets(s.h, wb.B, off1.ctypes.data_as(dp)) == 0
    ip = C.POINTER(C.c_int32)
    out = _poisoned(wb.B)
    rc = s.L.loc_window_marginal_prior_host(s.h, wb.B, wb.counts.ctypes.data_as(ip), wb.poses.ctypes.data_as(dp), wb.r_idx.ctypes.data_as(ip), wb.r_val.ctypes.data_as(dp),
                                            wb.p_idx.ctypes.data_as(ip), wb.p_val.ctypes.data_as(dp), wb.s_idx.ctypes.data_as(ip), wb.s_val.ctypes.data_as(dp),
                                            drop.ctypes.data_as(ip), out[0].ctypes.data_as(ip), out[1].ctypes.data_as(dp), out[2].ctypes.data_as(dp),
                                            out[3].ctypes.data_as(dp), out[4].ctypes.data_as(ip), out[5].ctypes.data_as(ip))
    assert rc == LOC_ERR_UNSUPPORTED and _untouched(out)
    assert s.L.loc_window_set_endpoint1_offsets(s.h, 0, None) == 0
    s.close()


def test_solves_before_and_after_are_unaffected(gpu):
    """the pass is stateless: the host path's next solve and the resident batch return what they return without it"""
    import localization_amd as la
    base, drop = F.case_batch(la, "fullprior")
    s = la.WindowSolver(ANCH, base.B, *base.caps, jacobian="numeric")
    first = base.copy()
    s.solve(first)
    kind = s.last_kernel_kind()
    s.upload(base)
    s.solve_resident()
    out = s.marginal_prior(first, drop)
    res = la.WindowBatch(base.B, *base.caps)
    s.download(res)
    second = base.copy()
    s.solve(second)
    assert s.last_kernel_kind() == kind
    again = s.marginal_prior(second, drop)
    s.close()
    used = np.arange(base.caps[0])[None, :] < base.counts[:, :1]
    assert np.array_equal(second.poses, first.poses) and np.array_equal(second.result, first.result)
    assert np.array_equal(res.poses[used], first.poses[used])
    for a, b in zip(out, again):
        assert np.array_equal(a, b)


# ---- the fixed-lag smoother: three slides of a window of six poses -----------------------------------------------------------------------------
W, SLIDES = 6, 3


def _fixed_lag_chains():
    return [F.Chain(7900 + i, W + SLIDES, 3 + i % 2) for i in range(8)]


@pytest.mark.parametrize("jac", ["analytic", "numeric"])
def test_fixed_lag_chain_against_the_oracle_chain(gpu, jac):
    """Solve, marginal prior of the oldest pose, slide, three times over.  The chain of windows is the GPU's; on every window the oracle
    solves a copy of it — the same start poses, the same carried prior row — so that each slide is ONE solve against one solve, held to
    the solve tolerances, and the numpy statement forms the marginal at the GPU's poses, held to the marginal's limits.  (Two chains that
    each follow their own unconverged ten-iteration iterates drift apart in numeric mode by more than one solve's tolerance: that would
    measure the accumulation of the difference quotient's noise, not a solve.)"""
    import localization_amd as la
    from oracle import oracle as O
    mode = _mode(O, jac)
    chains = _fixed_lag_chains()
    s = la.WindowSolver(ANCH, len(chains), *F.window_caps(W), jacobian=jac)
    g = F.first_window(la, chains, W)
    tol_max, tol_med = SOLVE_TOL[jac]
    for k in range(SLIDES + 1):
        o = g.copy()
        res = s.solve(g)
        assert k == 0 or s.last_kernel_kind() == "window_lm_kernel"   # (a carried prior has a full matrix: the general kernel)
        want_chi = np.zeros(o.B)
        for i in range(o.B):
            o.poses[i, :W], want_chi[i], _ = D.oracle_window(o, i, ANCH, 10, mode)
        dt = np.abs(g.poses[:, :, 9:] - o.poses[:, :, 9:])
        chi = np.abs(res[:, 0] - want_chi).max() / max(1.0, np.abs(want_chi).max())
        print(f"fixed lag {jac} window {k}: |gpu - oracle| max {dt.max():.3e} m, median {np.median(dt):.3e} m, chi2 relative {chi:.3e}")
        assert dt.max() < tol_max and np.median(dt) < tol_med and chi <= 1e-6, (k, dt.max(), np.median(dt), chi)
        if k == SLIDES:
            break
        out = s.marginal_prior(g, 0)
        slot, prior, status = out[0], out[1], out[5]
        assert not status.any() and (slot == 1).all()
        for i in range(g.B):
            assert _check_window(g, i, 0, D.marginal_ref(g, i, ANCH, mode, 0), out, jac, f"fixed lag slide {k + 1}") is not None
        g = F.next_window(la, g, chains, k + 1, W, slot, prior)
    s.close()


@pytest.mark.parametrize("jac", ["analytic", "numeric"])
def test_one_drop_property_with_the_gpus_own_prior(gpu, jac):
    """at a converged solve, the window shortened by its oldest pose stays where it was when that pose's marginal prior stands in for it,
    and moves a hundred times further without it"""
    import localization_amd as la
    chains = _fixed_lag_chains()
    s = la.WindowSolver(ANCH, len(chains), *F.window_caps(W), jacobian=jac, maximum_iteration=F.PROPERTY_ITERATIONS)
    wb = F.first_window(la, chains, W)
    s.solve(wb)
    slot, prior, _, _, _, status = s.marginal_prior(wb, 0)
    assert not status.any() and (slot == 1).all()
    moved = {}
    for with_prior in (True, False):
        short = la.WindowBatch(wb.B, *F.window_caps(W))
        for i, ch in enumerate(chains):
            F.add_chain_poses(short, i, ch, 1, W - 1, est=wb.poses[i, 1:W, 9:12])
            if with_prior:
                F.add_prior_row(short, i, 0, prior[i])
        s.solve(short)
        moved[with_prior] = np.abs(short.poses[:, :W - 1, 9:] - wb.poses[:, 1:W, 9:]).max(axis=(1, 2))
    s.close()
    print(f"one drop {jac}: kept poses move {moved[True]} m with the marginal prior, {moved[False]} m with the plain drop")
    assert (moved[True] < moved[False] / 100).all()
