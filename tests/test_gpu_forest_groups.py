"""GPU tests of option "forest_groups": a batch of forest windows whose topologies DIFFER — key-frame windows cut from different robots or at
different phases of the key cadence (Localization::addPoseEdge, localization.cpp:254-290) — on tree_wave_kernel<JAC, TreeGroups>, one
schedule per group of windows of one topology (tests/_forest_groups_cases.py builds the batches).

1. the bits of tree_wave_kernel on each group's windows gathered into a batch of their own (the same schedule, arithmetic and order: no
   tolerance); 2. the oracle, at the project's tolerances (poses 1e-7 analytic / 1e-5 numeric, chi2 1e-6 / 1e-4 relative);
3. what the option leaves alone; 4. the resident path, the topology cache, every window its own topology, one topology with other anchors."""
import numpy as np
import pytest

import _forest_groups_cases as FC
from _forest_groups_cases import ANCH, CAPS

pytestmark = pytest.mark.gpu

B, G = 70, 5
OF = [b % G for b in range(B)]          # neighbouring waves differ, and window B - 1 is not of group 0
GROUPS = "tree_wave_kernel<groups>"


def _solver(la, jac, groups=1, batch=B, **options):
    s = la.WindowSolver(ANCH, batch, *CAPS, jacobian=jac, bw_max=CAPS[0] - 1, chain_threshold=1)
    s.set_option("forest_groups", groups)                                    # (a library without the option refuses the name)
    for k, v in options.items():
        s.set_option(k, v)
    return s


def _same(a, b):
    """the poses of every window (the slots it uses: what lies behind a window's nv is not part of the answer — download() returns whatever the
    device array held there) and all eight result columns, bit for bit"""
    used = np.arange(a.caps[0])[None, :] < a.counts[:, :1]
    return np.array_equal(a.counts, b.counts) and np.array_equal(a.poses[used], b.poses[used]) and np.array_equal(a.result, b.result)


@pytest.mark.parametrize("jac", ["analytic", "numeric"])
def test_bits_of_tree_wave_kernel_on_each_group(gpu, jac):
    import localization_amd as la
    topos = FC.five_topologies()
    # the anchor choice varies per window inside a group: one anchor number is enough for build_tree_sched to decline the batch
    varied = FC.mixed_batch(la, topos, OF, 11)
    s = _solver(la, jac)
    s.solve(varied)
    assert s.last_kernel_kind() == GROUPS
    n, nbytes = s.forest_groups()
    assert n == G and nbytes > 0
    # tree_wave_kernel takes a group's windows only with equal anchor numbers and flags: the mixed batch rebuilt with those
    mixed = FC.mixed_batch(la, topos, OF, 11, vary=False)
    got = mixed.copy()
    res = s.solve(got).copy()
    assert s.last_kernel_kind() == GROUPS and s.forest_groups()[0] == G
    s.close()
    u = _solver(la, jac, groups=0)
    for g in range(G):
        rows = [b for b in range(B) if OF[b] == g]
        own = mixed.take(rows)
        want = u.solve(own).copy()
        assert u.last_kernel_kind() == "tree_wave_kernel" and u.forest_groups() == (0, 0)
        # poses and all eight result columns of every window, bit for bit — result[7] with the window's own nlev, nv and nroots
        assert np.array_equal(got.poses[rows], own.poses), (g, np.abs(got.poses[rows] - own.poses).max())
        assert np.array_equal(res[rows], want), (g, np.abs(res[rows] - want).max(axis=0))
        assert (want[:, 3] >= 1).all() and (want[:, 7] % 65536 >= 2 * topos[g]["T"] - 3).all()
    u.close()


@pytest.mark.parametrize("jac", ["analytic", "numeric"])
def test_mixed_batch_against_the_oracle(gpu, jac):
    """12 windows spread over the five groups, anchors and robust flags varying inside a group (the kernel reads each window's own rows).
    The random forest (group 4) is compared in analytic mode only: on deep random trees started 4 ... 8 cm off, tree_wave_kernel itself
    misses the numeric bound on a one-topology batch (tests/test_gpu_tree_parity.py:
    test_tree_wave_kernel_on_random_forests says why: the oracle's own two Jacobian modes end 1e-3 ... 1e-2 m apart there), and this
    kernel computes that kernel's bits.  The bound is not widened for it."""
    import localization_amd as la
    from oracle import oracle as O
    from _oracle_window import oracle_solve_instance
    topos = FC.five_topologies()
    wb = FC.mixed_batch(la, topos, OF, 12)
    windows = [0, 1, 2, 3, 4, 25, 26, 27, 28, 29, 68, 69]
    assert sorted(set(OF[b] for b in windows)) == list(range(G))
    if jac == "numeric":
        windows = [b for b in windows if OF[b] != 4]
    mode = O.JAC_ANALYTIC if jac == "analytic" else O.JAC_NUMERIC_G2O
    want = {b: oracle_solve_instance(wb, b, ANCH, jac_mode=mode) for b in windows}
    s = _solver(la, jac)
    res = s.solve(wb).copy()
    assert s.last_kernel_kind() == GROUPS and s.forest_groups()[0] == G
    s.close()
    tol, tol_chi = (1e-7, 1e-6) if jac == "analytic" else (1e-5, 1e-4)
    worst = []
    for b in windows:
        poses, chi, st = want[b]
        nv = int(wb.counts[b, 0])
        d = np.abs(wb.poses[b, :nv] - poses).max()
        c = abs(res[b, 0] - chi) / max(1.0, abs(chi))
        print(f"forest_groups oracle {jac}: window {b} group {OF[b]} |dpose| {d:.3e} chi2 rel {c:.3e} iterations {res[b, 3]:.0f} / {st.outer_iterations}")
        worst.append((d, c, b))
    for d, c, b in worst:
        assert d < tol and c <= tol_chi, (b, OF[b], d, c)


def test_the_option_leaves_everything_else_alone(gpu):
    import localization_amd as la
    topos = FC.five_topologies()
    mixed = FC.mixed_batch(la, topos, OF, 13)
    on, off = _solver(la, "analytic"), _solver(la, "analytic", groups=0)

    def both(wb, kind, **options):
        """wb on both handles under the same further options: the kernel that ran on each, and the bits"""
        a, b = wb.copy(), wb.copy()
        for s in (on, off):
            for k, v in options.items():
                s.set_option(k, v)
        on.solve(a); off.solve(b)
        assert (on.last_kernel_kind(), off.last_kernel_kind()) == (kind, kind), (on.last_kernel_kind(), off.last_kernel_kind(), options)
        assert on.forest_groups() == (0, 0)
        assert _same(a, b)

    # option off: the mixed batch is the general kernel's
    x = mixed.copy()
    off.solve(x)
    assert off.last_kernel_kind() == "window_lm_kernel" and off.forest_groups() == (0, 0)
    # a one-topology batch keeps today's path, kernel and bits
    both(FC.mixed_batch(la, topos, [2] * B, 14, vary=False), "tree_wave_kernel")
    # one window of the batch refuses all of it
    cyc = mixed.copy()
    cyc.add_range(7, 20, 33, 1.0, 10.0)                                       # window 7 (T = 40): a loop closure between two poses of one tree
    both(cyc, "window_lm_kernel")
    dbl = mixed.copy()
    vi, vj = (int(v) for v in dbl.s_idx[10, 5, :2])                           # window 10 (T = 64): a second EdgeSE3 on a pair that has one
    dbl.add_se3(10, vi, vj, np.zeros(3), np.eye(3), np.eye(6) * 2e3, True)
    both(dbl, "window_lm_kernel")
    # a table of full information matrices on the handle
    pin = mixed.copy()
    pin.p_info = np.zeros((B, CAPS[2], 36))
    pin.p_info[:, :, ::7] = pin.p_val[:, :, 12:]
    both(pin, "window_lm_kernel")
    # the lane-per-window variant has no twin; below the forest threshold nothing is grouped
    both(mixed, "window_lm_kernel", tree=2)
    both(mixed, "window_lm_kernel", tree=-1, chain_min_batch=B + 1)
    for s in (on, off):
        s.set_option("chain_min_batch", 1)
    # the grouped path again, then the covariances of the mixed batch: served as without the option, by the envelope pass
    y = mixed.copy()
    on.solve(y)
    assert on.last_kernel_kind() == GROUPS and on.forest_groups()[0] == G
    assert np.abs(y.poses - x.poses).max() < 1e-7                             # (and the general kernel's answer, at the kernels' tolerance)
    for s in (on, off):
        s.set_option("covariance_general", 1)
    cov_on, cov_off = on.covariance(y), off.covariance(y)
    assert all(np.array_equal(p, q, equal_nan=True) for p, q in zip(cov_on, cov_off)) and np.isfinite(cov_on[0][cov_on[2] == 0]).all()
    on.close(); off.close()


def test_resident_path_and_topology_cache(gpu):
    import localization_amd as la
    topos = FC.five_topologies()
    mixed = FC.mixed_batch(la, topos, OF, 15)
    s = _solver(la, "analytic")
    host = mixed.copy()
    res = s.solve(host).copy()
    assert s.last_kernel_kind() == GROUPS and not s.last_host_timing()[3]
    # the same structure again: the verdict, the groups and the tables come from the cache
    again = mixed.copy()
    s.solve(again)
    assert s.last_kernel_kind() == GROUPS and s.last_host_timing()[3] and s.forest_groups()[0] == G and _same(again, host)
    # resident: the host path's bits
    r = mixed.copy()
    s.upload(r)
    assert s.forest_groups()[0] == G
    s.solve_resident(); s.download(r)
    assert s.last_kernel_kind() == GROUPS and _same(r, host)
    # a host-path solve of ANOTHER mixed batch (other groups, other tables) does not disturb the resident one
    other = FC.mixed_batch(la, topos[:3], [(b * 2) % 3 for b in range(40)], 16)
    s.solve(other)
    assert s.last_kernel_kind() == GROUPS and s.forest_groups()[0] == 3 and not s.last_host_timing()[3]
    r.poses[:] = 0.0
    s.solve_resident(); s.download(r)
    assert s.last_kernel_kind() == GROUPS and _same(r, host)
    # a threshold raised after the upload is looked at per solve, as for every resident batch: the general kernel then
    s.set_option("chain_min_batch", B + 1)
    s.solve_resident(); s.download(r)
    used = np.arange(CAPS[0])[None, :] < r.counts[:, :1]
    assert s.last_kernel_kind() == "window_lm_kernel" and np.abs(r.poses[used] - host.poses[used]).max() < 1e-7
    s.close()


def test_every_window_its_own_topology_and_one_topology_with_other_anchors(gpu):
    import localization_amd as la
    # G = B: nv from 2 to 64, and the last seven windows repeat a length at another key cadence (another parent)
    own = [FC.star(2 + b, 5, n_anchor=2, lever=True) for b in range(63)] + [FC.star(10 + b, 2, n_anchor=2, lever=True) for b in range(B - 63)]
    wb = FC.mixed_batch(la, own, list(range(B)), 17)
    # G = 1: one topology, the anchors differ from every window to the next (and one robust flag in every third)
    one = FC.mixed_batch(la, [FC.star(40, 6, first=2)], [0] * B, 18)
    assert all((one.r_idx[b, :40, 1] != one.r_idx[b + 1, :40, 1]).all() for b in range(B - 1))
    g = _solver(la, "analytic", groups=0)
    s = _solver(la, "analytic")
    for batch, n_groups in ((wb, B), (one, 1)):
        ref, got = batch.copy(), batch.copy()
        g.solve(ref)
        res = s.solve(got)
        assert g.last_kernel_kind() == "window_lm_kernel" and s.last_kernel_kind() == GROUPS and s.forest_groups()[0] == n_groups
        d = np.abs(got.poses - ref.poses).max()
        print(f"forest_groups G = {n_groups}: |twin - window_lm_kernel| {d:.3e}")
        assert d < 1e-7
        nv = batch.counts[:, 0]
        assert ((res[:, 7] % 65536) == 2 * nv - 1).all()                      # one tree per window: 2 nv - nroots blocks, the window's own nv
    g.close(); s.close()
