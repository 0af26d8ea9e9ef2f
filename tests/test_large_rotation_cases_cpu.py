"""tests/_large_rotation_cases.py without a GPU: every window states the branches its factors take, and the oracle brings every
committed zero-residual window home (the gate tests/test_gpu_large_rotation_convergence.py applies again before it asks the kernels)."""
import numpy as np
import pytest

import _large_rotation_cases as L


@pytest.mark.parametrize("kind", L.KINDS)
def test_zero_residual_windows_start_in_every_branch_and_the_oracle_reaches_the_truth(built, kind):
    import localization_amd as la
    from oracle import oracle as O
    wb, truth = L.zero_residual_batch(la, kind)
    assert wb.B == 16
    L.assert_start_branches(wb, kind)
    for i in range(wb.B):   # zero residual at the truth: the measurements are the truth's own
        at = wb.poses[i].copy()
        wb.poses[i] = truth[i]
        _, chi, _ = L.oracle_solve(wb, i, L.ANCH, O.JAC_ANALYTIC, iterations=0)
        b = L.window_branches(wb, i)
        assert all(x == 0 for x in b["prior"] + b["se3_error"])
        wb.poses[i] = at
        assert chi < 1e-20, (i, chi)
        assert np.abs(np.linalg.norm(at[:, 9:] - truth[i, :, 9:], axis=1) - 0.05).max() < 1e-12
    for mode in (O.JAC_ANALYTIC, O.JAC_NUMERIC_G2O):
        L.oracle_gate(wb, truth, mode)


def test_evaluation_cases_cover_all_four_branches_of_every_conversion(built):
    """each case asserts its own windows' branches while it is built; together they reach every branch of the prior's error conversion, the
    EdgeSE3 error conversion and the two conversions of the EdgeSE3 Jacobian (the inverse measurement, Xi^T Xj)"""
    import localization_amd as la
    seen = {}
    for name in L.EVALUATION_CASES:
        wb, _, _, _ = L.evaluation_case(la, name)
        per = L.collect_branches(wb, seen)
        assert len(per) == wb.B
    for conv in ("prior", "se3_error", "se3_zinv", "se3_rel"):
        assert seen[conv] == {0, 1, 2, 3}, (conv, seen[conv])
    for what in ("chi2", "cov", "joint"):   # ... and so do the cases of each entry point alone
        part = {}
        for name, kinds in L.EVALUATION_CASES.items():
            if what in kinds:
                L.collect_branches(L.evaluation_case(la, name)[0], part)
        for conv in ("prior", "se3_error", "se3_zinv", "se3_rel"):
            assert part[conv] == {0, 1, 2, 3}, (what, conv, part[conv])
