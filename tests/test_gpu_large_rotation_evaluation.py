"""Single evaluations through the public entry points with every quaternion conversion in every branch: WindowSolver.edge_chi2 and
.covariance are stateless and evaluate at wb.poses, so they are called WITHOUT a solve on the existing generators' batches turned by the
two knobs of tests/_large_rotation_cases.py (estimates 60 .. 175 degrees off their priors about x, y, z and the diagonal; EdgeSE3
measurements of 125 .. 170 degrees, the estimates following them or not).  No LM decision is involved, so the existing references and
tolerances apply unchanged: tests/_edge_audit_ref.py with test_gpu_edge_audit's limit, tests/_covariance_ref.py with each covariance
file's own rule (relative Frobenius TOL, exact masks, symmetry, eigenvalue floor).  tests/test_oracle_kats.py pins those references'
linearisation to a 50-digit one in every branch.  Kernels reached: edge_audit_kernel.hip; covariance_kernel.hip (IMU priors, twist
EdgeSE3, 64 poses); forest_covariance_kernel.hip; envelope_covariance_kernel.hip (option covariance_general, also with full-information
priors).  joint_covariance launches the JOINT = true instantiations of those covariance kernels — separately compiled copies of the
conversions, and the cross-block path — so it has its own cases on the chain, twist, forest and envelope batches, held to
tests/test_gpu_joint_covariance.py's reference, block error and per-pass limits.  marginal_prior_kernel.hip serves translation-only
windows and converts no rotation: it has no case here."""
import numpy as np
import pytest

import _edge_audit_ref as R
import _large_rotation_cases as L

pytestmark = pytest.mark.gpu


def _solver(la, wb, anchors, ctor, opts, jac):
    s = la.WindowSolver(anchors, wb.B, *wb.caps, jacobian=jac, **ctor)
    for k, v in opts.items():
        s.set_option(k, v)
    return s


@pytest.mark.parametrize("name", [n for n, k in L.EVALUATION_CASES.items() if "chi2" in k])
def test_edge_chi2_in_every_branch(gpu, name):
    import localization_amd as la
    from test_gpu_edge_audit import _check_against_reference
    wb, anchors, ctor, opts = L.evaluation_case(la, name)
    s = _solver(la, wb, anchors, ctor, opts, "numeric")
    got = s.edge_chi2(wb)
    s.close()
    _check_against_reference(wb, anchors, got, "large rotations, " + name)


@pytest.mark.parametrize("jac", ["analytic", "numeric"])
@pytest.mark.parametrize("name", [n for n, k in L.EVALUATION_CASES.items() if "cov" in k])
def test_covariance_in_every_branch(gpu, name, jac):
    import localization_amd as la
    from oracle import oracle as O
    wb, anchors, ctor, opts = L.evaluation_case(la, name)
    s = _solver(la, wb, anchors, ctor, opts, jac)
    cov, mask, status = s.covariance(wb)
    s.close()
    if name == "cov_forest":
        from test_gpu_forest_covariance import _check
        worst = _check(O, wb, jac, cov, mask, status)
    elif name == "cov_envelope_table":   # full-information priors: test_gpu_dense_prior's reference (p_info honoured) and its rule
        import _dense_prior_ref as D
        from test_gpu_dense_prior import COV_TOL, KAPPA_EPS
        mode = O.JAC_ANALYTIC if jac == "analytic" else O.JAC_NUMERIC_G2O
        worst = 0.0
        for i in range(wb.B):
            nv = int(wb.counts[i, 0])
            assert status[i] == 0 and not mask[i].any() and not cov[i, nv:].any()
            want, want_mask, H = D.covariance_ref(wb, i, anchors, mode)
            assert not want_mask.any()
            tol = max(COV_TOL[jac], KAPPA_EPS * np.linalg.cond(H))
            for v in range(nv):
                err = np.linalg.norm(cov[i, v] - want[v]) / np.linalg.norm(want[v])
                worst = max(worst, err)
                assert err <= tol, (i, v, err, tol)
                assert np.array_equal(cov[i, v], cov[i, v].T)
                ev = np.linalg.eigvalsh(cov[i, v])
                assert ev.min() >= -1e-12 * ev.max()
    elif name.startswith("cov_envelope"):
        from test_gpu_general_covariance import _check
        worst = _check(O, wb, jac, cov, mask, status, name)
    else:
        from test_gpu_covariance import _check
        worst = _check(la, O, wb, jac, cov, mask, status)
    print(f"covariance at large rotations, {name} {jac}: max relative Frobenius error {worst:.3e}")


JOINT_PASS = {"cov_chain_imu": "chain", "cov_chain_twist": "chain", "cov_forest": "forest", "cov_envelope_chain6": "envelope"}


@pytest.mark.parametrize("jac", ["analytic", "numeric"])
@pytest.mark.parametrize("name", [n for n, k in L.EVALUATION_CASES.items() if "joint" in k])
def test_joint_covariance_in_every_branch(gpu, name, jac):
    """the cross blocks of adjacent, distant, repeated and transposed pose pairs (test_gpu_joint_covariance's own pair choices) and the
    marginals of the joint call, with every property its _check asserts"""
    import localization_amd as la
    import test_gpu_joint_covariance as J
    wb, anchors, ctor, opts = L.evaluation_case(la, name)
    pass_ = JOINT_PASS[name]
    per_window = (J._chain_pairs(wb) if pass_ == "chain" else J._forest_pairs(wb) if pass_ == "forest"
                  else J._outside_pairs(wb, lambda nv: [(0, nv - 1), (nv - 1, 0)]))
    pairs, counts = J._tables(wb, per_window)
    s = _solver(la, wb, anchors, ctor, opts, jac)
    plain = s.covariance(wb)
    joint = s.joint_covariance(wb, pairs, counts)
    s.close()
    J._check((wb, anchors, ctor, opts, pass_, per_window, (jac,)), jac, joint, plain, (pairs, counts), "large rotations, " + name)
