"""GPU tests of option "forest_groups_covariance": marginal pose covariances and the cross blocks of joint calls for batches of forest windows
whose topologies DIFFER, on forest_covariance_kernel<JAC, JOINT, TreeGroups> — one wave per window on the schedule of the window's group
(tests/_forest_groups_cov_cases.py builds the batches: six topologies, 72 windows).

1. the bits of forest_covariance_kernel on each group's windows gathered into a batch of their own (the same schedule, arithmetic and order:
   no tolerance); 2. the numpy reference of tests/_covariance_ref.py (marginals) and of the joint tests (cross blocks); 3. coverage and the
   switch; 4. the resident path, both table routes; 5. a singular window stays alone; 6. a topology per window, one topology with other anchors.

Tolerances.  Error of a marginal block: Frobenius norm of (GPU - reference) relative to the reference block's; of a cross
block: relative to sqrt(||R_ii|| ||R_jj||) (tests/_joint_cov_models.block_error).  analytic: the project's 1e-8.  numeric: 10x the largest
error of the EXISTING one-topology pass (forest_covariance_kernel, options off) on the gathered groups 1 - 5 of these inputs (vary off),
measured on an MI355X — by test 1 the new pass computes those bits —, capped at 1e-6.  Measured, marginal / cross: group 1 2.73e-13 /
2.72e-13, group 2 5.22e-13 / 2.10e-13, group 3 5.33e-13 / 5.05e-13, group 4 (a key with three leaves, smallest relative pivot 6.0e-5, kappa
4.5e5) 1.876e-11 / 1.873e-11, group 5 2.52e-12 / 2.52e-12; the analytic runs are at 3.9e-13 ... 2.8e-11 (group 4 again: the conditioning of H,
not the difference quotient).  The new pass on the vary-on batch of test 2: 7.90e-12 / 7.90e-12 numeric, 6.51e-12 / 6.51e-12 analytic.  A
window with kappa(H_kept) > 1e9 is held to max(limit, 1e-15 kappa), the forest file's rule (none here: kappa <= 6.3e5)."""
import functools

import numpy as np
import pytest

import _forest_groups_cases as FC
import _forest_groups_cov_cases as C
import _joint_cov_models as M
from _forest_groups_cov_cases import ANCH, B, CAPS, G, OF
from _covariance_ref import hessian
from test_gpu_joint_covariance import _forest_pairs, _tables

pytestmark = pytest.mark.gpu

LOC_ERR_UNSUPPORTED, LOC_ERR_SINGULAR = -5, -6
GROUPS_SOLVE = "tree_wave_kernel<groups>"
GROUPS, FOREST, ENVELOPE, CHAIN6 = "forest_covariance_kernel<groups>", "forest_covariance_kernel", "envelope_covariance_kernel", "covariance_kernel<6>"
TOL = {"analytic": 1e-8, "numeric": 1.9e-10}          # marginal blocks: 10 x 1.876e-11
TOL_CROSS = {"analytic": 1e-8, "numeric": 1.9e-10}    # cross blocks: 10 x 1.873e-11


def _solver(la, jac, groups=1, gcov=1, batch=B, **options):
    s = la.WindowSolver(ANCH, batch, *CAPS, jacobian=jac, bw_max=CAPS[0] - 1, chain_threshold=1)
    s.set_option("forest_groups", groups)
    s.set_option("forest_groups_covariance", gcov)                           # (a library without the option refuses the name)
    for k, v in options.items():
        s.set_option(k, v)
    return s


def _pairs(wb):
    """test_gpu_joint_covariance._forest_pairs' choice per window (parent - child in both orders, a diagonal, the ends, leaves of one key and of
    different keys, poses of different trees, the deepest poses), without the pairs that name a slot the window does not have (its (3, 3) in a
    window of two poses)"""
    per_window = _forest_pairs(wb, deepest=True)
    return [[p for p in ps if max(p) < int(wb.counts[w, 0])] for w, ps in enumerate(per_window)]


def _same(x, y):
    return all(np.array_equal(p, q, equal_nan=True) for p, q in zip(x, y, strict=True))


def _fresh(torch, gpu, n, npm=None):
    out = [torch.full((n, CAPS[0], 6, 6), 7.0, dtype=torch.float64, device=gpu), torch.full((n, CAPS[0]), 7, dtype=torch.int32, device=gpu),
           torch.full((n,), 7, dtype=torch.int32, device=gpu)]
    if npm is not None:
        out.append(torch.full((n, npm, 6, 6), 7.0, dtype=torch.float64, device=gpu))
    return out


def _host(ts):
    return tuple(t.cpu().numpy() for t in ts)


@functools.lru_cache(maxsize=None)
def _solved(jac, vary):
    """(the mixed batch at the GPU's poses, the plain call's outputs, the joint call's, the pair tables) on a handle with both options on;
    shared, never modified"""
    import localization_amd as la
    wb = C.mixed(la, vary)
    s = _solver(la, jac)
    s.solve(wb)
    assert s.last_kernel_kind() == GROUPS_SOLVE and s.forest_groups()[0] == G
    assert s.last_covariance_kind() == "none"
    plain = s.covariance(wb)
    assert s.last_covariance_kind() == GROUPS and s.last_covariance_ms() > 0
    pairs, counts = _tables(wb, _pairs(wb))
    joint = s.joint_covariance(wb, pairs, counts)
    assert s.last_covariance_kind() == GROUPS
    assert s.last_kernel_kind() == GROUPS_SOLVE and s.forest_groups()[0] == G      # (a covariance call leaves both reports alone)
    s.close()
    return wb, plain, joint, (pairs, counts)


@pytest.mark.parametrize("jac", ["analytic", "numeric"])
def test_bits_of_forest_covariance_kernel_on_each_group(gpu, jac):
    """Groups 1 - 5 gathered: a batch of ONE topology, which a handle without the options serves on forest_covariance_kernel.  The two-pose
    windows (group 6) are left out here and only here: a batch of them alone is a chain and takes the chain pass."""
    import localization_amd as la
    wb, plain, joint, (pairs, counts) = _solved(jac, False)
    assert _same(plain, joint[:3])                                            # the marginals of a joint call are the plain call's
    assert not plain[2].any()
    u = _solver(la, jac, groups=0, gcov=0)
    for g in range(5):
        rows = [b for b in range(B) if OF[b] == g]
        own = wb.take(rows)
        want = u.covariance(own)
        assert u.last_covariance_kind() == FOREST
        assert _same([x[rows] for x in plain], want), g
        want = u.joint_covariance(own, pairs[rows], counts[rows])
        assert u.last_covariance_kind() == FOREST
        assert _same([x[rows] for x in joint], want), g
        assert counts[rows].min() >= 4 and np.abs(want[3]).max() > 0
    u.close()


def _reference(wb, jac):
    """per window: (Sigma on the kept coordinates, keep, kappa) of the reference's H at wb.poses"""
    from oracle import oracle as O
    mode = O.JAC_ANALYTIC if jac == "analytic" else O.JAC_NUMERIC_G2O
    out = []
    for i in range(wb.B):
        H = hessian(wb, i, ANCH, mode)
        Sig, keep = M.kept_inverse(H)
        out.append((Sig, keep, np.linalg.cond(H[np.ix_(keep, keep)]), C.min_relative_pivot(H)))
    return out


def _check(wb, jac, ref, cov, mask, status, cross=None, tables=None, tol=None, tol_cross=None):
    """test_gpu_forest_covariance._check's properties for every window (status, zero blocks behind nv, the mask, every block against the
    reference, exact symmetry, PSD, zero rows / columns of excluded coordinates), and test_gpu_joint_covariance._check's for the cross
    blocks.  Returns the largest errors."""
    tol = TOL[jac] if tol is None else tol
    tol_cross = TOL_CROSS[jac] if tol_cross is None else tol_cross
    worst, worst_cross, at = 0.0, 0.0, None
    for i in range(wb.B):
        nv = int(wb.counts[i, 0])
        Sig, keep, kappa, _ = ref[i]
        assert status[i] == 0, (i, status[i])
        assert not cov[i, nv:].any() and not mask[i, nv:].any()
        want_mask = np.array([sum(1 << k for k in range(6) if not keep[6 * v + k]) for v in range(nv)], dtype=np.int32)
        assert np.array_equal(mask[i, :nv], want_mask), (i, mask[i, :nv], want_mask)
        lim = tol if kappa <= 1e9 else max(tol, 1e-15 * kappa)
        for v in range(nv):
            g, r = cov[i, v], M.blk(Sig, v, v)
            assert np.linalg.norm(r) > 0
            err = np.linalg.norm(g - r) / np.linalg.norm(r)
            if err > worst:
                worst, at = err, (i, v)
            assert err <= lim, (i, v, err, lim, kappa)
            assert np.array_equal(g, g.T)
            ev = np.linalg.eigvalsh(g)
            assert ev.min() >= -1e-12 * ev.max()
            for k in range(6):
                if (mask[i, v] >> k) & 1:
                    assert not g[k].any() and not g[:, k].any()
        if cross is None:
            continue
        pairs, counts = tables
        n = int(counts[i])
        assert not cross[i, n:].any()
        limc = tol_cross if kappa <= 1e9 else max(tol_cross, 1e-15 * kappa)
        seen = {}
        for p in range(n):
            a, b = int(pairs[i, p, 0]), int(pairs[i, p, 1])
            g = cross[i, p]
            err = M.block_error(g, Sig, a, b)
            worst_cross = max(worst_cross, err)
            assert err <= limc, (i, (a, b), err, limc, kappa)
            for k in range(6):
                if (mask[i, a] >> k) & 1: assert not g[k].any()
                if (mask[i, b] >> k) & 1: assert not g[:, k].any()
            if a == b: assert np.array_equal(g, cov[i, a])
            if (a, b) in seen: assert np.array_equal(g, seen[(a, b)])
            if (b, a) in seen: assert np.array_equal(g, seen[(b, a)].T)
            seen[(a, b)] = g
            if not M.blk(Sig, a, b).any(): assert not g.any()             # poses of different trees: exact zeros
    return worst, worst_cross, at


@pytest.mark.parametrize("jac", ["analytic", "numeric"])
def test_parity_with_the_reference(gpu, jac):
    """all six topologies, anchors and robust flags varying inside a group (the kernel reads each window's own rows)"""
    wb, plain, joint, tables = _solved(jac, True)
    assert _same(plain, joint[:3])
    ref = _reference(wb, jac)
    pivot, kappa = min(r[3] for r in ref), max(r[2] for r in ref)
    worst, worst_cross, at = _check(wb, jac, ref, *joint, tables=tables)
    print(f"forest groups covariance {jac}: max marginal error {worst:.3e} (window {at[0]} group {OF[at[0]]} pose {at[1]}), limit {TOL[jac]:.1e}; "
          f"max cross error {worst_cross:.3e}, limit {TOL_CROSS[jac]:.1e}; smallest relative pivot {pivot:.2e}, largest kappa {kappa:.2e}")
    # the inputs are regular by the reference alone: every LDL^T pivot above 1e-9 of its diagonal entry, two orders clear of the 1e-11 rule
    assert pivot > 1e-9
    rich = [b for b in range(B) if OF[b] == 1]
    cross = joint[3]
    for b in rich[:2]:                                                        # two trees (0 ... 14, 15 ... 23): the pair (0, nv - 1) joins them
        p = _pairs(wb)[b].index((0, 23))
        assert not cross[b, p].any() and cross[b, 0].any()


def _untouched(la, s, wb):
    out = (np.full((wb.B, CAPS[0], 6, 6), 7.0), np.full((wb.B, CAPS[0]), 7, dtype=np.int32), np.full(wb.B, 7, dtype=np.int32))
    with pytest.raises(la.LocalizationAmdError) as ex:
        s.covariance(wb, out=out)
    assert ex.value.code == LOC_ERR_UNSUPPORTED
    assert (out[0] == 7.0).all() and (out[1] == 7).all() and (out[2] == 7).all()


def test_coverage_and_the_switch(gpu):
    import localization_amd as la
    wb, plain, _, _ = _solved("analytic", True)
    s = _solver(la, "analytic", gcov=0)
    _untouched(la, s, wb)                                                     # the option off, no envelope pass: not covered
    assert s.last_covariance_kind() == "none"
    s.set_option("covariance_general", 1)
    env = s.covariance(wb)
    assert s.last_covariance_kind() == ENVELOPE
    for general in (1, 0):                                                    # the option on: the new pass under either value
        s.set_option("covariance_general", general)
        s.set_option("forest_groups_covariance", 1)
        assert _same(s.covariance(wb), plain) and s.last_covariance_kind() == GROUPS
    # (the envelope pass sums in another order: the two passes agree at the analytic tolerance, not bit for bit)
    used = np.arange(CAPS[0])[None, :] < wb.counts[:, :1]
    assert np.array_equal(env[1], plain[1]) and not env[2].any()
    assert (np.linalg.norm(env[0][used] - plain[0][used], axis=(1, 2)) <= 1e-8 * np.linalg.norm(plain[0][used], axis=(1, 2))).all()

    def falls_back(batch, **options):
        """under `options` the batch is the envelope pass's with "covariance_general", and refused without; afterwards the new pass again"""
        restore = {"forest_groups": 1, "tree": -1, "chain_min_batch": 1}
        for k, v in options.items():
            s.set_option(k, v)
        s.set_option("covariance_general", 0)
        _untouched(la, s, batch)
        s.set_option("covariance_general", 1)
        got = s.covariance(batch)
        assert s.last_covariance_kind() == ENVELOPE, options
        for k in options:
            s.set_option(k, restore[k])
        return got

    assert _same(falls_back(wb, forest_groups=0), env)
    falls_back(wb, tree=0)
    falls_back(wb, tree=2)
    falls_back(wb, chain_min_batch=B + 1)
    pin = wb.copy()                                                           # a table of full information matrices on the handle
    pin.p_info = np.zeros((B, CAPS[2], 36))
    pin.p_info[:, :, ::7] = pin.p_val[:, :, 12:]
    falls_back(pin)
    cyc = wb.copy()
    assert OF[8] == 2
    cyc.add_range(8, 20, 33, 1.0, 10.0)                                       # window 8 (T = 40): a loop closure between two poses of one tree
    falls_back(cyc)
    dbl = wb.copy()
    assert OF[6] == 0
    vi, vj = (int(v) for v in dbl.s_idx[6, 5, :2])                            # window 6 (T = 64): a second EdgeSE3 on a pair that has one
    dbl.add_se3(6, vi, vj, np.zeros(3), np.eye(3), np.eye(6) * 2e3, True)
    falls_back(dbl)
    assert _same(s.covariance(wb), plain) and s.last_covariance_kind() == GROUPS   # (wb's own table, none, is the handle's again)
    s.close()


def test_other_batches_keep_their_pass_and_the_solves_their_bits(gpu):
    import localization_amd as la
    from test_gpu_covariance import _twist_batch
    topos = C.six_topologies()
    on, off = _solver(la, "numeric"), _solver(la, "numeric", groups=0, gcov=0)
    one = FC.mixed_batch(la, topos, [2] * 16, 43, vary=False)                 # a one-topology batch
    on.solve(one)
    assert _same(on.covariance(one), off.covariance(one)) and on.last_covariance_kind() == off.last_covariance_kind() == FOREST
    ch = _twist_batch(la, np.random.default_rng(500 + 15 + len("twist_robust") + len("numeric")), 24, 15, True)   # test_gpu_forest_covariance.test_coverage_rule's chain batch
    a, b = la.WindowSolver(ANCH, 24, *ch.caps, jacobian="numeric", chain_threshold=1), la.WindowSolver(ANCH, 24, *ch.caps, jacobian="numeric", chain_threshold=1)
    a.set_option("forest_groups", 1); a.set_option("forest_groups_covariance", 1)
    a.solve(ch)
    assert _same(a.covariance(ch), b.covariance(ch)) and a.last_covariance_kind() == b.last_covariance_kind() == CHAIN6
    a.close(); b.close()
    # a handle that computes covariances between its solves returns the solve's bits and the same forest_groups() as one that never does
    wb = C.mixed(la, True)
    other = FC.mixed_batch(la, topos[:3], [(k * 2) % 3 for k in range(40)], 44)
    never = _solver(la, "numeric")
    wa, wc = wb.copy(), wb.copy()
    for rep in range(2):
        ra = on.solve(wa).copy()
        on.covariance(wa); on.covariance(other)
        assert on.last_covariance_kind() == GROUPS and on.forest_groups()[0] == G   # (the covariance of a batch of three groups does not touch the report)
        rb = never.solve(wc).copy()
        assert np.array_equal(wa.poses, wc.poses) and np.array_equal(ra, rb)
        assert on.last_kernel_kind() == never.last_kernel_kind() == GROUPS_SOLVE and on.forest_groups() == never.forest_groups() and on.forest_groups()[0] == G
        assert on.last_host_timing()[3] == never.last_host_timing()[3]       # (the topology cache: a hit on both from the second round on)
        wa.poses[:, :, 9:] += 0.01; wc.poses[:, :, 9:] += 0.01
    on.close(); off.close(); never.close()


@pytest.mark.parametrize("route", ["uploaded_block", "option_after_upload", "own_block"])
def test_resident_matches_host_bit_for_bit(gpu, route):
    """uploaded_block: both options on at the upload — the covariance pass walks the resident solve's groups block; option_after_upload: the
    same with "forest_groups_covariance" set only afterwards; own_block: uploaded with "forest_groups" 0 (the general kernel solves it), both
    options switched on afterwards — the first call classifies the batch and builds a block of its own."""
    import torch
    import localization_amd as la
    wb = C.mixed(la, True)
    pairs, counts = _tables(wb, _pairs(wb))
    npm = pairs.shape[1]
    s = _solver(la, "numeric", groups=0 if route == "own_block" else 1, gcov=1 if route == "uploaded_block" else 0)
    s.upload(wb)
    s.solve_resident()
    solve_kind = "window_lm_kernel" if route == "own_block" else GROUPS_SOLVE
    assert s.last_kernel_kind() == solve_kind
    if route != "uploaded_block":
        out = _fresh(torch, gpu, B)
        with pytest.raises(la.LocalizationAmdError) as ex:                    # not covered yet
            s.covariance_resident(*out)
        assert ex.value.code == LOC_ERR_UNSUPPORTED and all((t == 7).all() for t in out)
        s.set_option("forest_groups", 1)
        s.set_option("forest_groups_covariance", 1)
    plain_d = _fresh(torch, gpu, B)
    s.covariance_resident(*plain_d)
    assert s.last_covariance_kind() == GROUPS and s.last_covariance_ms() > 0
    joint_d = _fresh(torch, gpu, B, npm)
    s.joint_covariance_resident(pairs, counts, *joint_d)
    other = torch.cuda.Stream(device=gpu)
    plain_e, joint_e = _fresh(torch, gpu, B), _fresh(torch, gpu, B, npm)
    torch.cuda.synchronize()
    s.covariance_resident(*plain_e, stream=other)
    s.joint_covariance_resident(pairs, counts, *joint_e, stream=other)
    other.synchronize()
    got = wb.copy()
    s.download(got)
    plain = s.covariance(got)
    joint = s.joint_covariance(got, pairs, counts)
    assert s.last_covariance_kind() == GROUPS and not plain[2].any()
    for t in (plain_d, plain_e):
        assert _same(_host(t), plain)
    for t in (joint_d, joint_e):
        assert _same(_host(t), joint)
    # off and on again under "covariance_general": the envelope pass, then the new pass
    s.set_option("covariance_general", 1)
    s.set_option("forest_groups_covariance", 0)
    env_d = _fresh(torch, gpu, B)
    s.covariance_resident(*env_d)
    assert s.last_covariance_kind() == ENVELOPE
    s.set_option("forest_groups_covariance", 1)
    back_d = _fresh(torch, gpu, B)
    s.covariance_resident(*back_d)
    torch.cuda.synchronize()                                                  # (the call is asynchronous on the handle's own stream)
    assert s.last_covariance_kind() == GROUPS and _same(_host(back_d), plain)
    # the resident batch is still there: another solve + download gives the same poses
    again = wb.copy()
    s.solve_resident()
    s.download(again)
    used = np.arange(CAPS[0])[None, :] < wb.counts[:, :1]
    assert np.array_equal(again.poses[used], got.poses[used])
    assert s.last_kernel_kind() == solve_kind                                 # (own_block: the upload did not group, whatever "forest_groups" is now)
    s.close()


def test_singular_window_is_isolated(gpu):
    """One window of a group keeps its structure but loses the information of all its range rows: a gauge-free forest, H singular —
    LOC_ERR_SINGULAR and NaN; every other window, the others of its group included, is bit-identical to the batch without the change."""
    import localization_amd as la
    wb, plain, joint, (pairs, counts) = _solved("numeric", True)
    bad = wb.copy()
    i = 24                                                                    # group 0, with eleven others
    assert OF[i] == 0
    bad.r_val[i, :, 1] = 0.0
    s = _solver(la, "numeric")
    got = s.joint_covariance(bad, pairs, counts)
    assert s.last_covariance_kind() == GROUPS
    s.close()
    assert got[2][i] == LOC_ERR_SINGULAR and np.isnan(got[0][i]).all() and np.isnan(got[3][i, :counts[i]]).all()
    others = [k for k in range(B) if k != i]
    assert not got[2][others].any()
    assert _same([x[others] for x in got], [x[others] for x in joint])


def test_every_window_its_own_topology_and_one_topology_with_other_anchors(gpu):
    """G = B (every window another length; 61 windows: star(4 + b, 5) up to the handle's 64 poses) and G = 1, against the envelope pass at the
    analytic tolerance"""
    import localization_amd as la
    NB = CAPS[0] - 3                                                          # 61 windows of 4 ... 64 poses: every length the handle takes, once
    own = FC.mixed_batch(la, [FC.star(4 + b, 5, n_anchor=2, lever=True) for b in range(NB)], list(range(NB)), 45)
    one = FC.mixed_batch(la, [C.six_topologies()[2]], [0] * B, 46)
    assert all((one.r_idx[b, :40, 1] != one.r_idx[b + 1, :40, 1]).all() for b in range(B - 1))
    s = _solver(la, "analytic")
    e = _solver(la, "analytic", gcov=0, covariance_general=1)
    for batch, n_groups in ((own, NB), (one, 1)):
        s.solve(batch)
        assert s.last_kernel_kind() == GROUPS_SOLVE and s.forest_groups()[0] == n_groups
        got, want = s.covariance(batch), e.covariance(batch)
        assert s.last_covariance_kind() == GROUPS and e.last_covariance_kind() == ENVELOPE
        assert not got[2].any() and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
        used = np.arange(CAPS[0])[None, :] < batch.counts[:, :1]
        err = np.linalg.norm(got[0][used] - want[0][used], axis=(1, 2)) / np.linalg.norm(want[0][used], axis=(1, 2))
        print(f"forest groups covariance G = {n_groups}: max |new pass - envelope pass| relative {err.max():.3e}")
        assert err.max() <= TOL["analytic"]
        assert not got[0][~used].any()
    s.close(); e.close()
