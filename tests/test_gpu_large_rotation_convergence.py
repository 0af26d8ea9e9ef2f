"""Every 6-DoF LM kernel from a start in the quaternion branches the parity tests never reach: zero-residual windows
(tests/_large_rotation_cases.py) whose unique minimum is the ground truth whatever path LM takes, started 150 degrees off about x, y
or z or 170 degrees off about the diagonal, 5 cm off in translation.  The expected value is the truth, not a solver's output: the
oracle only GATES the inputs (it must reach the truth to 1e-12 within the same 40 iterations, for every window), then the kernel must
reach it to 1e-9 m and 1e-9 per rotation entry — two orders inside what the parity suite asks of noisy solves, six above what the
oracle leaves — and report chi2 <= 1e-12.  A wrong branch in a kernel's own error or Jacobian code shows as rejected steps or a wrong
fixed point; last-bit differences are for tests/test_gpu_device_primitives.py and tests/test_gpu_large_rotation_evaluation.py.
Whole-solve parity at such starts is deliberately not tested."""
import numpy as np
import pytest

import _large_rotation_cases as L

pytestmark = pytest.mark.gpu

T = 5
# (the kernel the batch must take, the windows, constructor arguments, handle options) — selected as the parity tests select them
VERDICTS = {
    "window": ("window_lm_kernel", "chain", dict(chain_threshold=0), {}),
    "window_pinfo": ("window_lm_kernel", "chain_pinfo", dict(chain_threshold=0), {}),        # evaluate_edges<.., PINFO>
    "chain": ("chain_lm_kernel", "chain", dict(chain_threshold=1), {}),
    "chain_se3": ("chain_lm_kernel", "twist", dict(chain_threshold=1), {}),
    "tree_wave": ("tree_wave_kernel", "forest", dict(chain_threshold=1, bw_max=T - 1), {}),
    "tree_lane": ("tree_lm_kernel", "forest", dict(chain_threshold=1, bw_max=T - 1), {"tree": 2}),
    "wave6": ("wave6_lm_kernel", "chain", {}, {}),
    "wave6_se3": ("wave6_lm_kernel<SE3>", "twist", {}, {}),
}


@pytest.mark.parametrize("jac", ["analytic", "numeric"])
@pytest.mark.parametrize("verdict", sorted(VERDICTS))
def test_kernel_reaches_the_truth_from_every_branch(gpu, verdict, jac):
    import localization_amd as la
    from oracle import oracle as O
    kernel, kind, ctor, opts = VERDICTS[verdict]
    wb, truth = L.zero_residual_batch(la, kind, T=T)
    L.assert_start_branches(wb, kind)
    mode = O.JAC_ANALYTIC if jac == "analytic" else O.JAC_NUMERIC_G2O
    L.oracle_gate(wb, truth, mode, iterations=40)
    s = la.WindowSolver(L.ANCH, wb.B, *wb.caps, maximum_iteration=40, jacobian=jac, **ctor)
    for k, v in opts.items():
        s.set_option(k, v)
    start = wb.poses.copy()
    res = s.solve(wb).copy()
    assert s.last_kernel_kind() == kernel, s.last_kernel_kind()
    s.close()
    gaps = np.array([L.truth_gap(wb.poses[i], truth[i]) for i in range(wb.B)])
    print(f"convergence {verdict} {jac}: max |t - truth| {gaps[:, 0].max():.3e} m, max |R - truth| {gaps[:, 1].max():.3e}, "
          f"max chi2 {res[:, 0].max():.3e}, iterations {int(res[:, 3].min())} .. {int(res[:, 3].max())}")
    for i in range(wb.B):
        if not (gaps[i, 0] <= 1e-9 and gaps[i, 1] <= 1e-9 and res[i, 0] <= 1e-12):   # the kernel's result row next to the oracle's statistics
            wb.poses[i] = start[i]
            _, chi, st = L.oracle_solve(wb, i, L.ANCH, mode, iterations=40)
            print(f"  window {i}: gap {gaps[i]}, result {res[i]}; oracle: chi2 {chi:.3e}, iterations {st.outer_iterations}, "
                  f"trials {st.lm_trials}, terminated {st.terminated}, lambda {st.lambda_:.3e}")
    assert (gaps[:, 0] <= 1e-9).all() and (gaps[:, 1] <= 1e-9).all(), gaps.max(axis=0)
    assert (res[:, 0] <= 1e-12).all(), res[:, 0].max()
