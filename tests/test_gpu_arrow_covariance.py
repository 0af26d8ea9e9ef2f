"""GPU checks of the marginal covariances of ARROWHEAD windows (anchor self-calibration: arrow_covariance_kernel.hip through
loc_window_covariance_host / _resident) against the numpy reference of tests/_covariance_ref.py, at the estimates the solve returns:
every slot, tag poses and unknown anchors alike.  Definition: DESIGN.md §2, tolerances and measured values: DESIGN.md §3.

Inputs: tests/_arrow_cov_inputs.py (test_gpu_arrow3_parity._arrow_batch's windows with at least four ranged nodes per tag pose; the surveyed
anchors are that file's FIXED and two more).  Every input meant to pass is regular by the reference alone (tests/test_arrow_covariance_cpu.py
at the oracle-solved poses; test_inputs_are_regular_by_the_reference repeats it at the GPU's poses).

Tolerance: relative Frobenius error per block as test_gpu_covariance._check computes it, limit that file's TOL, relaxed per window to
KAPPA_EPS * kappa(H_kept) (test_gpu_snapshot_covariance.KAPPA_EPS: the first-order bound of an inverse) where that is larger — the weak
anchor priors (information 1 beside ranges of 330) make these H worse conditioned than a chain's."""
import numpy as np
import pytest

from test_gpu_arrow3_parity import FIXED
from test_gpu_covariance import TOL
from test_gpu_snapshot_covariance import KAPPA_EPS
from _arrow_cov_inputs import CASES, SURVEYED, arrow_cov_batch, case_batch, cut_gauge, min_relative_pivot
from _covariance_ref import hessian, reference_covariance

pytestmark = pytest.mark.gpu

LOC_ERR_UNSUPPORTED, LOC_ERR_SINGULAR = -5, -6
KERNEL = "arrow3_lm_kernel"


def _solver(la, wb, jac, arrow3=1):
    s = la.WindowSolver(SURVEYED, wb.B, *wb.caps, jacobian=jac)
    if arrow3 is not None:
        s.set_option("arrow3", arrow3)
    return s


def _check(O, wb, jac, cov, mask, status):
    mode = O.JAC_ANALYTIC if jac == "analytic" else O.JAC_NUMERIC_G2O
    worst, worst_ratio, kmax = 0.0, 0.0, 0.0
    for i in range(wb.B):
        nv = int(wb.counts[i, 0])
        assert status[i] == 0, (i, status[i])
        assert not cov[i, nv:].any() and not mask[i, nv:].any()
        want, want_mask = reference_covariance(wb, i, SURVEYED, mode)
        assert np.array_equal(mask[i, :nv], want_mask), (i, mask[i, :nv], want_mask)
        assert ((mask[i, :nv] & 0x38) == 0x38).all()          # translation-only: every rotation coordinate excluded
        H = hessian(wb, i, SURVEYED, mode)
        keep = np.diag(H) != 0
        kappa = np.linalg.cond(H[np.ix_(keep, keep)])
        kmax = max(kmax, kappa)
        tol = max(TOL[jac], KAPPA_EPS * kappa)
        for v in range(nv):
            g, r = cov[i, v], want[v]
            nr = np.linalg.norm(r)
            assert nr > 0
            err = np.linalg.norm(g - r) / nr
            worst = max(worst, err); worst_ratio = max(worst_ratio, err / tol)
            assert err <= tol, (i, v, err, tol, kappa)
            assert np.array_equal(g, g.T)
            ev = np.linalg.eigvalsh(g)
            assert ev.min() >= -1e-12 * ev.max()
            for k in range(6):
                if (mask[i, v] >> k) & 1:
                    assert not g[k].any() and not g[:, k].any()
    return worst, worst_ratio, kmax


PARITY = [(name, jac) for name in CASES for jac in CASES[name][4]]


@pytest.mark.parametrize("name,jac", PARITY)
def test_parity_with_the_reference(gpu, name, jac):
    import localization_amd as la
    from oracle import oracle as O
    wb = case_batch(la, name)
    assert np.array_equal(SURVEYED[:2], FIXED)
    s = _solver(la, wb, jac, CASES[name][3])
    s.solve(wb)
    assert s.last_kernel_kind() == KERNEL
    cov, mask, status = s.covariance(wb)
    assert s.last_covariance_ms() > 0
    assert s.last_kernel_kind() == KERNEL
    s.close()
    worst, ratio, kappa = _check(O, wb, jac, cov, mask, status)
    print(f"arrow covariance {name} {jac}: max relative Frobenius error {worst:.3e} ({ratio:.3f} of its limit), largest kappa {kappa:.3e}")


@pytest.mark.parametrize("name", list(CASES))
def test_inputs_are_regular_by_the_reference(gpu, name):
    """Every LDL^T pivot of the reference's H_kept is above 1e-9 of its diagonal entry at the solved poses: two orders clear of the 1e-11
    rule, so no window of the parity cases is near the singular verdict."""
    import localization_amd as la
    from oracle import oracle as O
    wb = case_batch(la, name)
    s = _solver(la, wb, "numeric", CASES[name][3])
    s.solve(wb)
    assert s.last_kernel_kind() == KERNEL
    s.close()
    for i in range(wb.B):
        assert min_relative_pivot(hessian(wb, i, SURVEYED, O.JAC_NUMERIC_G2O)) > 1e-9, i


def test_singular_window_is_isolated(gpu):
    """One window keeps its structure but loses the information of its anchor priors and of its ranges to surveyed anchors: nothing holds the
    gauge, H is singular (the reference's smallest relative pivot is below 1e-12) — LOC_ERR_SINGULAR and NaN; the other windows are
    bit-identical to the batch without the change."""
    import localization_amd as la
    from oracle import oracle as O
    B = 5
    wb = arrow_cov_batch(la, np.random.default_rng(9300), B, 24, 4, False)
    s = _solver(la, wb, "numeric")
    s.solve(wb)
    cov0, mask0, st0 = s.covariance(wb)
    assert (st0 == 0).all()
    bad = wb.copy()
    i = 2
    cut_gauge(bad, i)
    assert min_relative_pivot(hessian(bad, i, SURVEYED, O.JAC_NUMERIC_G2O)) < 1e-12
    cov, mask, st = s.covariance(bad)
    s.close()
    nv = int(bad.counts[i, 0])
    assert st[i] == LOC_ERR_SINGULAR and np.isnan(cov[i, :nv]).all() and not cov[i, nv:].any()
    others = [k for k in range(B) if k != i]
    assert (st[others] == 0).all()
    assert np.array_equal(cov[others], cov0[others]) and np.array_equal(mask[others], mask0[others])


def _untouched(la, s, wb):
    out = (np.full((wb.B, wb.caps[0], 6, 6), 7.0), np.full((wb.B, wb.caps[0]), 7, dtype=np.int32), np.full(wb.B, 7, dtype=np.int32))
    with pytest.raises(la.LocalizationAmdError) as ex:
        s.covariance(wb, out=out)
    assert ex.value.code == LOC_ERR_UNSUPPORTED
    assert (out[0] == 7.0).all() and (out[1] == 7).all() and (out[2] == 7).all()


def test_coverage_rule(gpu):
    """Served iff the handle would solve the batch on arrow3_lm_kernel: option "arrow3" (default: windows of more than 64 poses only),
    translation-only, build_arrow_aux's structure test; chains as before."""
    import localization_amd as la
    from test_gpu_covariance import ANCH, _observable_batch
    small = arrow_cov_batch(la, np.random.default_rng(9500), 2, 24, 4, False)      # 28 poses
    s = _solver(la, small, "analytic", None)
    _untouched(la, s, small)                              # default handle: the wave-per-window kernel solves it
    s.set_option("arrow3", 1)
    cov, mask, st = s.covariance(small)                   # whenever the batch qualifies: served
    assert (st == 0).all() and np.isfinite(cov).all() and cov[:, :, 0, 0].all()
    s.set_option("arrow3", 0)
    _untouched(la, s, small)                              # never
    s.close()
    big = arrow_cov_batch(la, np.random.default_rng(9501), 2, 70, 4, False)        # 74 poses: the default rule serves it
    s = _solver(la, big, "analytic", None)
    cov, mask, st = s.covariance(big)
    assert (st == 0).all() and np.isfinite(cov).all() and cov[:, :, 0, 0].all()

    # the mutations of test_arrow3_is_taken_by_large_translation_only_arrowheads_only
    def lever(wb): wb.r_val[1, 5, 2:5] = (0.0, 0.01, 0.0)
    def turned(wb): wb.poses[0, 3, :9] = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]]).reshape(9)
    def second_link(wb): wb.add_range(0, 10, 11, 0.01, 50.0)           # two edges on one consecutive chain pair
    def long_link(wb): wb.add_range(0, 10, 40, 1.0, 50.0)              # a loop closure inside the chain: the border would be 34 poses
    for mut in (lever, turned, second_link, long_link):
        wb = big.copy()
        mut(wb)
        _untouched(la, s, wb)
    s.set_option("arrow3", 0)
    _untouched(la, s, big)
    s.close()
    # a chain batch still runs the chain pass: the same bits with option "arrow3" = 1 as on a default handle
    ch = _observable_batch(la, np.random.default_rng(9502), 6, 10, False, False, translation_only=True)
    a, b = la.WindowSolver(ANCH, 6, *ch.caps, jacobian="numeric"), la.WindowSolver(ANCH, 6, *ch.caps, jacobian="numeric")
    b.set_option("arrow3", 1)
    a.solve(ch)
    ca, cb = a.covariance(ch), b.covariance(ch)
    assert (ca[2] == 0).all() and all(np.array_equal(x, y) for x, y in zip(ca, cb))
    a.close(); b.close()


@pytest.mark.parametrize("classified_by", ["upload", "first_call"])
def test_resident_matches_host_bit_for_bit(gpu, classified_by):
    """upload, solve_resident, covariance_resident into torch buffers (twice: the second call takes the cached classification; on another
    stream), download, and the host path at the downloaded poses: the same bits.  first_call: the upload was not classified as an arrowhead
    (option "arrow3" was 0 then), so the first covariance call scans the uploaded tables."""
    import torch
    import localization_amd as la
    wb = case_batch(la, "24_4")
    B, T = wb.B, wb.caps[0]
    s = _solver(la, wb, "numeric", 0 if classified_by == "first_call" else 1)
    s.upload(wb)
    s.set_option("arrow3", 1)
    s.solve_resident()
    assert s.last_kernel_kind() == (KERNEL if classified_by == "upload" else "window_lm_kernel")

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
    assert np.array_equal(wb.poses, before)
    assert s.last_kernel_kind() == (KERNEL if classified_by == "upload" else "window_lm_kernel")
    s.close()


def test_solves_are_unaffected(gpu):
    """A handle that computes covariances between its solves — of the batch it solves and of an arrowhead of another shape — returns the same
    bits (poses, results, kernel kind) as one that never does, on the host path and resident."""
    import torch
    import localization_amd as la
    wb = case_batch(la, "24_4")
    B, T = wb.B, wb.caps[0]
    other = arrow_cov_batch(la, np.random.default_rng(9600), B, 24, 4, False)
    a, b = _solver(la, wb, "numeric"), _solver(la, wb, "numeric")
    wa, wc = wb.copy(), wb.copy()
    for rep in range(3):
        ra = a.solve(wa).copy()
        a.covariance(wa)
        a.covariance(other)
        assert a.last_kernel_kind() == KERNEL
        rb = b.solve(wc).copy()
        assert np.array_equal(wa.poses, wc.poses) and np.array_equal(ra, rb)
        assert a.last_kernel_kind() == b.last_kernel_kind() == KERNEL
        wa.poses[:, :, 9:] += 0.01; wc.poses[:, :, 9:] += 0.01
    wa, wc = wb.copy(), wb.copy()
    a.upload(wa); b.upload(wc)
    out = (torch.zeros((B, T, 36), dtype=torch.float64, device=gpu), torch.zeros((B, T), dtype=torch.int32, device=gpu), torch.zeros((B,), dtype=torch.int32, device=gpu))
    for rep in range(2):
        a.solve_resident(); b.solve_resident()
        a.covariance_resident(*out)
        a.covariance(other)
        ra, rb = a.download(wa).copy(), b.download(wc).copy()
        # (slots >= nv of a ragged resident batch are never written by the solve: the download returns whatever the device array held)
        assert all(np.array_equal(wa.poses[i, :nv], wc.poses[i, :nv]) for i, nv in enumerate(wb.counts[:, 0])) and np.array_equal(ra, rb)
        assert a.last_kernel_kind() == b.last_kernel_kind() == KERNEL
    a.close(); b.close()
