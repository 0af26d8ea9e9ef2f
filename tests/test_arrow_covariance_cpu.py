"""CPU checks behind the arrowhead covariance (arrow_covariance_kernel.hip), on the oracle alone: the inputs of
tests/test_gpu_arrow_covariance.py are regular at the oracle-solved poses, and the block identity the kernel rests on holds in numpy."""
import numpy as np
import pytest

from _arrow_cov_inputs import CASES, MIN_NODES, SURVEYED, arrow_cov_batch, case_batch, cut_gauge, min_relative_pivot, ranged_nodes
from _covariance_ref import hessian, reference_covariance
from _oracle_window import oracle_solve_instance


def _solved(wb, mode):
    out = wb.poses.copy()
    for i in range(wb.B):
        nv = int(wb.counts[i, 0])
        out[i, :nv] = oracle_solve_instance(wb, i, SURVEYED, jac_mode=mode)[0]
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_inputs_are_regular_at_the_oracle_solved_poses(built, name):
    """Every tag pose ranges at least four nodes, every unknown anchor carries a prior, and at the oracle-solved poses every LDL^T pivot of
    the reference's H_kept is above 1e-9 of its diagonal entry: two orders clear of the kernel's 1e-11 rule."""
    import localization_amd as la
    from oracle import oracle as O
    wb = case_batch(la, name)
    T, A = CASES[name][:2]
    assert wb.counts[:, 0].max() == T + A
    for jac in CASES[name][4]:
        mode = O.JAC_ANALYTIC if jac == "analytic" else O.JAC_NUMERIC_G2O
        poses = _solved(wb, mode)
        for i in range(wb.B):
            nodes, anchors = ranged_nodes(wb, i)
            assert min(nodes) >= MIN_NODES and len(anchors) >= 1, (i, nodes)
            assert anchors == list(range(int(wb.counts[i, 0]) - len(anchors), int(wb.counts[i, 0])))
            piv = min_relative_pivot(hessian(wb, i, SURVEYED, mode, poses[i]))
            assert piv > 1e-9, (name, jac, i, piv)


def test_a_window_without_gauge_is_singular_by_the_reference(built):
    """The singular case of the GPU test: without its anchor priors and its ranges to surveyed anchors a window floats freely — the reference's
    smallest relative pivot is below 1e-12."""
    import localization_amd as la
    from oracle import oracle as O
    wb = arrow_cov_batch(la, np.random.default_rng(9300), 3, 24, 4, False)
    wb.poses[:] = _solved(wb, O.JAC_NUMERIC_G2O)
    i = 1
    assert min_relative_pivot(hessian(wb, i, SURVEYED, O.JAC_NUMERIC_G2O)) > 1e-9
    bad = wb.copy()
    cut_gauge(bad, i)
    assert min_relative_pivot(hessian(bad, i, SURVEYED, O.JAC_NUMERIC_G2O)) < 1e-12


@pytest.mark.parametrize("jac", ["analytic", "numeric"])
def test_block_identity(built, jac):
    """H = [A B; B^T C] with the chain first and the border (the unknown anchors) last, Y = A^-1 B, S = C - B^T Y:
    [H^-1]_ii = [A^-1]_ii + Y_i S^-1 Y_i^T for a chain pose and [H^-1]_border = S^-1 — against reference_covariance, translation blocks."""
    import localization_amd as la
    from oracle import oracle as O
    mode = O.JAC_ANALYTIC if jac == "analytic" else O.JAC_NUMERIC_G2O
    wb = arrow_cov_batch(la, np.random.default_rng(9400), 3, 9, 3, True)
    wb.poses[:] = _solved(wb, mode)
    for i in range(wb.B):
        nv = int(wb.counts[i, 0])
        _, anchors = ranged_nodes(wb, i)
        nc = nv - len(anchors)
        want, mask = reference_covariance(wb, i, SURVEYED, mode)
        assert (mask == 0x38).all()
        H6 = hessian(wb, i, SURVEYED, mode)
        tr = np.array([6 * v + k for v in range(nv) for k in range(3)])
        H = H6[np.ix_(tr, tr)]
        Am, Bm, Cm = H[:3 * nc, :3 * nc], H[:3 * nc, 3 * nc:], H[3 * nc:, 3 * nc:]
        for a in range(nc):   # A is block-tridiagonal: the chain
            for b in range(nc):
                if abs(a - b) > 1:
                    assert not Am[3 * a:3 * a + 3, 3 * b:3 * b + 3].any()
        Ai = np.linalg.inv(Am)
        Y = Ai @ Bm
        Si = np.linalg.inv(Cm - Bm.T @ Y)
        for v in range(nc):
            Yv = Y[3 * v:3 * v + 3]
            got = Ai[3 * v:3 * v + 3, 3 * v:3 * v + 3] + Yv @ Si @ Yv.T
            assert np.linalg.norm(got - want[v][:3, :3]) <= 1e-9 * np.linalg.norm(want[v]), (i, v)
        for b in range(nv - nc):
            got = Si[3 * b:3 * b + 3, 3 * b:3 * b + 3]
            assert np.linalg.norm(got - want[nc + b][:3, :3]) <= 1e-9 * np.linalg.norm(want[nc + b]), (i, b)
