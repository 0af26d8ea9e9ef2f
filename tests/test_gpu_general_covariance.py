"""GPU checks of the marginal pose covariances of windows of GENERAL structure and of long windows (envelope_covariance_kernel.hip through
loc_window_covariance_host / _resident with option "covariance_general" = 1) against the numpy reference of tests/_covariance_ref.py, at the
estimates the solve returns.  Definition: DESIGN.md §2, tolerances and measured values: DESIGN.md §3.

Inputs: tests/_general_cov_inputs.py; every input meant to pass is regular by the reference alone (tests/test_general_covariance_cpu.py at
the oracle-solved poses).

Tolerance: relative Frobenius error per block as test_gpu_covariance._check computes it.  analytic: the project's 1e-8.  numeric: 10x the
largest value measured over every case of this file on an MI355X (DESIGN.md §3 lists every case).  A block is held to
max(tolerance, KAPPA_EPS * kappa(H_kept)) (test_gpu_snapshot_covariance.KAPPA_EPS: the first-order bound of an inverse).  In numeric mode
that raises the limit of every window with kappa > 8.4e3 — most 6-DoF windows here, up to 3.0e-10 on the tall stars (kappa 3.0e5); in
analytic mode it never applies.  No measured error needs it: every block is below 8.4e-12."""
import functools

import numpy as np
import pytest

from test_gpu_snapshot_covariance import KAPPA_EPS
import _general_cov_inputs as G
from _covariance_ref import hessian, reference_covariance

pytestmark = pytest.mark.gpu

LOC_ERR_UNSUPPORTED, LOC_ERR_SINGULAR = -5, -6
TOL = {"analytic": 1e-8, "numeric": 8.4e-12}
ANCH = G.ANCH


def _solver(la, wb, jac, general=1, **kw):
    s = la.WindowSolver(ANCH, wb.B, *wb.caps, jacobian=jac, **kw)
    s.set_option("covariance_general", general)
    return s


def _check(O, wb, jac, cov, mask, status, label):
    """test_gpu_covariance._check's assertions, every window and every block, with the kappa rule"""
    mode = O.JAC_ANALYTIC if jac == "analytic" else O.JAC_NUMERIC_G2O
    worst, kmax, relaxed = 0.0, 0.0, False
    for i in range(wb.B):
        nv = int(wb.counts[i, 0])
        assert status[i] == 0, (i, status[i])
        assert not cov[i, nv:].any() and not mask[i, nv:].any()
        want, want_mask = reference_covariance(wb, i, ANCH, mode)
        assert np.array_equal(mask[i, :nv], want_mask), (i, mask[i, :nv], want_mask)
        H = hessian(wb, i, ANCH, mode)
        keep = np.diag(H) != 0
        kappa = np.linalg.cond(H[np.ix_(keep, keep)])
        kmax = max(kmax, kappa)
        tol = max(TOL[jac], KAPPA_EPS * kappa)
        relaxed = relaxed or tol > TOL[jac]
        errs = []
        for v in range(nv):
            g, r = cov[i, v], want[v]
            nr = np.linalg.norm(r)
            assert nr > 0
            errs.append(np.linalg.norm(g - r) / nr)
            assert np.array_equal(g, g.T)
            ev = np.linalg.eigvalsh(g)
            assert ev.min() >= -1e-12 * ev.max()
            for k in range(6):
                if (mask[i, v] >> k) & 1:
                    assert not g[k].any() and not g[:, k].any()
        print(f"general covariance {label} {jac} window {i}: max relative Frobenius error {max(errs):.3e}, kappa {kappa:.3e}, limit {tol:.3e}")
        worst = max(worst, max(errs))
        assert max(errs) <= tol, (i, int(np.argmax(errs)), max(errs), tol, kappa)
    print(f"general covariance {label} {jac}: max relative Frobenius error {worst:.3e}, largest kappa {kmax:.3e}, kappa rule applies: {relaxed}")
    return worst


def _same_poses(wa, wc):
    """the poses of two batches agree bit for bit in every used slot (a download leaves the slots >= nv as the device has them)"""
    used = np.arange(wa.caps[0])[None, :] < wa.counts[:, :1]
    return np.array_equal(wa.poses[used], wc.poses[used])


@functools.lru_cache(maxsize=None)
def _solved(name, jac):
    """(batch at the GPU's poses, its covariances through the host entry point) of a parity case; shared, never modified"""
    import localization_amd as la
    wb = G.case_batch(la, name)
    s = _solver(la, wb, jac)
    s.solve(wb)
    out = s.covariance(wb)
    assert s.last_covariance_ms() > 0
    s.close()
    return wb, out


PARITY = [(name, jac) for name in G.CASES for jac in G.CASES[name][1]]


@pytest.mark.parametrize("name,jac", PARITY)
def test_parity_with_the_reference(gpu, name, jac):
    from oracle import oracle as O
    wb, (cov, mask, status) = _solved(name, jac)
    _check(O, wb, jac, cov, mask, status, name)
    nv = wb.counts[:, 0]
    if name.startswith("chain3"):   # translation-only: the rotation bits come from the exactly-zero rule
        for i in range(wb.B):
            assert ((mask[i, :nv[i]] & 0x38) == 0x38).all() and not cov[i, :, 3:, :].any() and not cov[i, :, :, 3:].any()
    if name == "mixed":
        assert tuple(int(x) for x in nv) == G.MIXED_NV
        assert (mask[3, G.MIXED_NV[3] - 3:G.MIXED_NV[3]] == 0x38).all() and not mask[3, :G.MIXED_NV[3] - 3].any()   # the unknown anchors' rotations


@pytest.mark.parametrize("jac", ["analytic", "numeric"])
def test_agrees_with_the_chain_pass(gpu, jac):
    """Twelve-pose 6-DoF chain windows on a handle of 65 pose slots (the envelope pass) and on one of 64 (covariance_kernel<6>)."""
    import localization_amd as la
    from oracle import oracle as O
    out = {}
    poses = None
    for nv_max in (64, 65):
        wb = G.chain_batch(la, 9301, 8, 12, True, nv_max=nv_max)
        s = _solver(la, wb, jac)
        if poses is None:
            s.solve(wb)
            poses = wb.poses.copy()
        else:
            wb.poses[:, :64] = poses                    # both passes at the same estimates: the 64-slot handle's solve
        out[nv_max] = (wb, s.covariance(wb))
        s.close()
    (wa, (ca, ma, sa)), (wc, (cc, mc, sc)) = out[65], out[64]
    _check(O, wa, jac, ca, ma, sa, "chains of 12 on 65 slots")
    assert np.array_equal(ma[:, :64], mc) and np.array_equal(sa, sc) and not sa.any()
    worst = 0.0
    for i in range(wa.B):
        for v in range(int(wa.counts[i, 0])):
            worst = max(worst, np.linalg.norm(ca[i, v] - cc[i, v]) / np.linalg.norm(cc[i, v]))
    print(f"envelope pass against covariance_kernel<6> {jac}: max relative Frobenius difference {worst:.3e}")
    assert worst <= TOL[jac]


def test_structured_batches_keep_their_kernels(gpu):
    """With the option on, a chain batch of <= 64 poses, an arrowhead batch and a forest batch return the bits they return with it off."""
    import localization_amd as la
    from _arrow_cov_inputs import SURVEYED, case_batch as arrow_case
    from test_gpu_forest_covariance import _case as forest_case

    def both(anchors, wb, setup, **kw):
        res = []
        for general in (0, 1):
            s = la.WindowSolver(anchors, wb.B, *wb.caps, jacobian="numeric", **kw)
            setup(s)
            s.set_option("covariance_general", general)
            w2 = wb.copy()
            s.solve(w2)
            res.append(s.covariance(w2))
            s.close()
        assert not res[0][2].any()
        assert all(np.array_equal(x, y) for x, y in zip(*res))

    both(ANCH, G.chain_batch(la, 9302, 6, 20, True), lambda s: None)
    both(SURVEYED, arrow_case(la, "24_4"), lambda s: s.set_option("arrow3", 1))
    wb, _ = forest_case(la, "plain_33_5")
    both(ANCH, wb, lambda s: None, bw_max=wb.caps[0] - 1, chain_threshold=1)


def test_singular_window_is_isolated(gpu):
    """One window of the mixed batch — the leaves-first star — loses every range: a gauge-free tree, H singular.  LOC_ERR_SINGULAR and NaN
    in its nv blocks; every other window's bits are unchanged."""
    import localization_amd as la
    from oracle import oracle as O
    wb, (cov0, mask0, st0) = _solved("mixed", "numeric")
    bad = wb.copy()
    i = G.MIXED_STAR
    bad.counts[i, 1] = 0
    assert G.min_relative_pivot(hessian(bad, i, ANCH, O.JAC_NUMERIC_G2O)) < 1e-12
    s = _solver(la, wb, "numeric")
    cov, mask, st = s.covariance(bad)
    s.close()
    nv = int(bad.counts[i, 0])
    assert st[i] == LOC_ERR_SINGULAR and np.isnan(cov[i, :nv]).all() and not cov[i, nv:].any()
    others = [k for k in range(wb.B) if k != i]
    assert (st[others] == 0).all()
    assert np.array_equal(cov[others], cov0[others]) and np.array_equal(mask[others], mask0[others])


@pytest.mark.parametrize("name", ["mixed", "chain3_130"])
def test_resident_matches_host_bit_for_bit(gpu, name):
    """covariance_resident = covariance(wb) at the downloaded poses: right after the solve, again with no solve in between, after another
    solve, and on a second stream; the solve outputs equal those of a handle that never computes a covariance."""
    import torch
    import localization_amd as la
    wb = G.case_batch(la, name)
    B, T = wb.B, wb.caps[0]
    a, b = _solver(la, wb, "numeric"), la.WindowSolver(ANCH, B, *wb.caps, jacobian="numeric")
    wa, wc = wb.copy(), wb.copy()
    a.upload(wa); b.upload(wc)
    a.solve_resident(); b.solve_resident()

    def fresh():
        return (torch.full((B, T, 6, 6), 7.0, dtype=torch.float64, device=gpu), torch.full((B, T), 7, dtype=torch.int32, device=gpu),
                torch.full((B,), 7, dtype=torch.int32, device=gpu))

    outs = [fresh()]
    a.covariance_resident(*outs[0])
    assert a.last_covariance_ms() > 0
    outs.append(fresh())
    a.covariance_resident(*outs[1])                       # no solve in between
    a.solve_resident(); b.solve_resident()
    outs.append(fresh())
    a.covariance_resident(*outs[2])                       # a solve in between
    other = torch.cuda.Stream(device=gpu)
    outs.append(fresh())
    torch.cuda.synchronize()
    a.covariance_resident(*outs[3], stream=other)
    other.synchronize()
    ra, rb = a.download(wa).copy(), b.download(wc).copy()
    assert _same_poses(wa, wc) and np.array_equal(ra, rb) and a.last_kernel_kind() == b.last_kernel_kind()
    cov, mask, st = a.covariance(wa)
    assert not st.any()
    for c, m, t in outs:
        assert np.array_equal(c.cpu().numpy(), cov) and np.array_equal(m.cpu().numpy(), mask) and np.array_equal(t.cpu().numpy(), st)
    # interleaved host-path calls leave the host solve alone as well
    w1, w2 = wb.copy(), wb.copy()
    r1 = a.solve(w1).copy(); a.covariance(w1); r1b = a.solve(wb.copy()).copy()
    r2 = b.solve(w2).copy()
    assert _same_poses(w1, w2) and np.array_equal(r1, r2) and np.array_equal(r1b, r2)
    a.close(); b.close()


def test_option_off_again(gpu):
    """After set_option("covariance_general", 0) the same handle refuses the batch again and writes nothing, host and resident."""
    import torch
    import localization_amd as la
    wb = G.case_batch(la, "mixed")
    s = _solver(la, wb, "numeric")
    s.upload(wb)
    s.solve_resident()
    out_d = (torch.full((wb.B, 24, 36), 7.0, dtype=torch.float64, device=gpu), torch.full((wb.B, 24), 7, dtype=torch.int32, device=gpu),
             torch.full((wb.B,), 7, dtype=torch.int32, device=gpu))
    s.covariance_resident(*out_d)
    s.download(wb)
    first = [t.cpu().numpy().copy() for t in out_d]
    assert not first[2].any()
    s.set_option("covariance_general", 0)
    for t in out_d: t.fill_(7)
    torch.cuda.synchronize()
    with pytest.raises(la.LocalizationAmdError) as ex:
        s.covariance_resident(*out_d)
    assert ex.value.code == LOC_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert all((t == 7).all().item() for t in out_d)
    out = (np.full((wb.B, 24, 6, 6), 7.0), np.full((wb.B, 24), 7, dtype=np.int32), np.full(wb.B, 7, dtype=np.int32))
    with pytest.raises(la.LocalizationAmdError) as ex:
        s.covariance(wb, out=out)
    assert ex.value.code == LOC_ERR_UNSUPPORTED
    assert (out[0] == 7.0).all() and (out[1] == 7).all() and (out[2] == 7).all()
    s.set_option("covariance_general", 1)                 # and on again: the resident batch is classified anew
    s.covariance_resident(*out_d)
    torch.cuda.synchronize()
    assert all(np.array_equal(t.cpu().numpy(), f) for t, f in zip(out_d, first))
    with pytest.raises(la.LocalizationAmdError) as ex:
        s.set_option("covariance_general", 2)
    assert ex.value.code == -1
    s.close()


def test_resident_batch_follows_the_structured_switches(gpu):
    """A resident forest batch below the forest threshold is the envelope pass's; once the threshold admits it, the forest pass takes it
    again, and back — after every change the resident call gives the bits of the host call, which classifies every time."""
    import torch
    import localization_amd as la
    from test_gpu_forest_covariance import _case as forest_case
    wb, _ = forest_case(la, "plain_33_5")
    B, T = wb.B, wb.caps[0]
    s = _solver(la, wb, "numeric", bw_max=T - 1)          # the default threshold: twelve windows are no forest batch
    f = la.WindowSolver(ANCH, B, *wb.caps, jacobian="numeric", bw_max=T - 1, chain_threshold=1)   # forest pass, option off
    s.upload(wb)
    s.solve_resident()
    s.download(wb)
    forest = f.covariance(wb)
    f.close()
    seen = []
    for threshold in (-1, 1, -1):
        s.set_option("chain_min_batch", threshold)
        out = (torch.full((B, T, 6, 6), 7.0, dtype=torch.float64, device=gpu), torch.full((B, T), 7, dtype=torch.int32, device=gpu),
               torch.full((B,), 7, dtype=torch.int32, device=gpu))
        torch.cuda.synchronize()
        s.covariance_resident(*out)
        torch.cuda.synchronize()
        res = [t.cpu().numpy() for t in out]
        assert not res[2].any()
        assert all(np.array_equal(x, y) for x, y in zip(res, s.covariance(wb)))
        seen.append(res)
    assert all(np.array_equal(x, y) for x, y in zip(seen[1], forest))      # the forest kernel's bits while the threshold admits the batch
    assert all(np.array_equal(x, y) for x, y in zip(seen[0], seen[2]))
    s.close()


def test_endpoint1_lever_arms_stay_unsupported(gpu):
    import localization_amd as la
    wb = G.chain_batch(la, 9303, 2, 70, False)
    wb.r_off1 = np.zeros((2, wb.caps[1], 3)); wb.r_off1[:, :, 0] = 0.1
    s = _solver(la, wb, "numeric")
    s.upload(wb)
    s.solve_resident()
    import torch
    out_d = (torch.full((2, 70, 36), 7.0, dtype=torch.float64, device=gpu), torch.full((2, 70), 7, dtype=torch.int32, device=gpu),
             torch.full((2,), 7, dtype=torch.int32, device=gpu))
    with pytest.raises(la.LocalizationAmdError) as ex:
        s.covariance_resident(*out_d)
    assert ex.value.code == LOC_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert all((t == 7).all().item() for t in out_d)
    s.close()


def test_plan_matches_the_pass(gpu):
    """covariance_plan(wb) is what the pass needs: its block count is the numpy count of the largest envelope, its bytes follow the header's
    formula, and the pass runs every window of a batch whose largest envelope belongs to ONE window (the key-first star) inside it."""
    import localization_amd as la
    wb, (cov, mask, st) = _solved("mixed", "analytic")
    s = _solver(la, wb, "analytic")
    blocks, nbytes = s.covariance_plan(wb)
    s.close()
    assert blocks == max(G.envelope_blocks(wb, i) for i in range(wb.B)) == 20 * 21 // 2
    assert nbytes == wb.B * ((blocks + 24) * 36 + 24 * 6) * 8
    assert not st.any() and np.isfinite(cov).all()
