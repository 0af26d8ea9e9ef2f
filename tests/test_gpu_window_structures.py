"""window_lm_kernel against the CPU oracle on the structures its analysis tells apart and the reference's node never builds: loops, grids,
cliques, several components, arrowheads with and without a pendant pose, a banded window on the skyline path (tests/_graph_families.py).

Every batch is pinned to the general kernel and solved in both Jacobian modes, 10 iterations, against oracle_solve_instance in the same mode,
with the tolerances of tests/test_gpu_window_parity.py (analytic 1e-7 m / 1e-7 on rotation entries, chi2 1e-6 relative; numeric 1e-5, 1e-4).
tests/test_graph_families_cpu.py shows that the reference alone stays a factor 10 inside them on every window (no LM decision at a rounding
edge), tests/test_elimination_model_cpu.py that every window takes the branch it is here for.  Per window:
  1. poses, chi2 and outer iterations = the oracle's; slots beyond the window untouched;
  2. result[7] = levels * 65536 + blocks (+ root poses / 16) of tests/_elimination_model.py; result[6] = the binary edges on shared pairs;
  3. the relabelled batch gives the same poses (1e-9 analytic — the bound of test_elimination_order_is_transparent —, the numeric tolerance
     in numeric mode) and the structure the model gives for the relabelled graph;
  4. the caller's order (natural_order) likewise;
  5. upload / solve_resident / download gives the bits of the host path.
Measured distances: DESIGN.md §3."""
import numpy as np
import pytest

import _elimination_model as M
import _graph_families as F
from _general_cov_inputs import ANCH, window_pairs

pytestmark = pytest.mark.gpu
CASES = [(name, mode) for name in F.BATCHES for mode in F.batch_modes(name)]


def _solver(la, caps, B, mode, natural=False):
    s = la.WindowSolver(ANCH, B, *caps[:4], maximum_iteration=10, bw_max=caps[4], jacobian=mode, natural_order=natural, chain_threshold=0)
    for opt in ("arrow3", "tree", "wave3", "wave6", "chain3"):
        s.set_option(opt, 0)
    return s


def _want7(wb, i, caps, natural=False):
    m = M.model_for(int(wb.counts[i, 0]), window_pairs(wb, i), caps, natural)
    return 0.0 if m is None else M.result7(m)      # (the skyline path reports no structure)


@pytest.mark.parametrize("name,mode", CASES)
def test_structures_match_oracle(gpu, name, mode):
    import localization_amd as la
    caps = F.batch_caps(name)
    tol, tol_chi = F.TOL[mode]
    tol_same = 1e-9 if mode == "analytic" else tol
    wb = F.build_batch(name)
    B, nvs = wb.B, [int(x) for x in wb.counts[:, 0]]
    before = wb.poses.copy()
    solver = _solver(la, caps, B, mode)
    res = solver.solve(wb).copy()
    assert solver.last_kernel_kind() == "window_lm_kernel"
    assert np.isfinite(wb.poses).all() and np.isfinite(res).all()
    want = F.oracle_solution(name, mode)
    for i, nv in enumerate(nvs):
        poses, chi2, outer, trials = want[i]
        d = np.abs(wb.poses[i, :nv] - poses)
        dchi = abs(res[i, 0] - chi2) / max(1.0, abs(chi2))
        print(f"{name} {mode} {F.BATCHES[name][3][i][0]}: |t| {d[:, 9:].max():.2e} |R| {d[:, :9].max():.2e} (limit {tol:.0e}) chi2 {dchi:.2e} (limit {tol_chi:.0e}) "
              f"outer {int(res[i, 3])}/{outer} trials {int(res[i, 4])}/{trials} result[7] {res[i, 7]}")
        assert d.max() < tol and dchi <= tol_chi, (name, mode, i, d[:, 9:].max(), d[:, :9].max(), dchi, res[i, 3:5], outer, trials)
        assert res[i, 3] == outer
        assert res[i, 7] == _want7(wb, i, caps) and res[i, 6] == F.shared_edges(wb, i), (name, i, res[i, 6:], _want7(wb, i, caps))
        assert np.array_equal(wb.poses[i, nv:], before[i, nv:])

    # 5. the resident path: the same bits
    wr = F.build_batch(name)
    solver.upload(wr)
    solver.solve_resident()
    solver.download(wr)
    assert solver.last_kernel_kind() == "window_lm_kernel"
    assert np.array_equal(wr.result, res)
    for i, nv in enumerate(nvs):     # (the slots beyond a window: the host path leaves the caller's, download() returns the device's — unspecified)
        assert np.array_equal(wr.poses[i, :nv], wb.poses[i, :nv]), (name, i)

    # 3. the relabelled batch
    wp = F.relabelled_batch(name)
    resp = solver.solve(wp).copy()
    assert solver.last_kernel_kind() == "window_lm_kernel"
    solver.close()
    for i, perm in enumerate(F.batch_perms(name)):
        d = np.abs(wp.poses[i, perm] - wb.poses[i, :nvs[i]]).max()
        print(f"{name} {mode} {F.BATCHES[name][3][i][0]}: relabelled {d:.2e} (limit {tol_same:.0e}) result[7] {resp[i, 7]}")
        assert d < tol_same and abs(resp[i, 0] - res[i, 0]) <= tol_chi * max(1.0, abs(res[i, 0])), (name, mode, i, d)
        assert resp[i, 3] == res[i, 3] and resp[i, 6] == res[i, 6] and resp[i, 7] == _want7(wp, i, caps), (name, i, resp[i], _want7(wp, i, caps))

    # 4. the caller's order
    if name in F.NATURAL:
        wn = F.build_batch(name)
        solver = _solver(la, caps, B, mode, natural=True)
        resn = solver.solve(wn).copy()
        assert solver.last_kernel_kind() == "window_lm_kernel"
        solver.close()
        for i, nv in enumerate(nvs):
            d = np.abs(wn.poses[i, :nv] - wb.poses[i, :nv]).max()
            print(f"{name} {mode} {F.BATCHES[name][3][i][0]}: natural order {d:.2e} (limit {tol_same:.0e}) result[7] {resn[i, 7]}")
            assert d < tol_same and abs(resn[i, 0] - res[i, 0]) <= tol_chi * max(1.0, abs(res[i, 0])), (name, mode, i, d)
            assert resn[i, 3] == res[i, 3] and resn[i, 6] == res[i, 6] and resn[i, 7] == _want7(wn, i, caps, True), (name, i, resn[i], _want7(wn, i, caps, True))
