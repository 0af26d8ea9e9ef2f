"""GPU checks of the joint marginals (loc_window_joint_covariance_host / _resident: the cross blocks [H^-1]_ij of requested pose pairs, on
the chain, forest, arrowhead and envelope passes) against the numpy reference of tests/_covariance_ref.py at the estimates the solve
returns: H there, its exactly-zero coordinates dropped, np.linalg.inv, block (i, j).  Definition: DESIGN.md §2, tolerances and measured
values: DESIGN.md §3.

Inputs: the existing builders only (test_gpu_covariance._observable_batch / _twist_batch, test_gpu_forest_covariance._case,
tests/_arrow_cov_inputs.py, tests/_general_cov_inputs.py), so every window is regular by the reference alone; none is left out of any
comparison.  Batches of the shared builders that come with more than eight windows are cut to their first eight.

Error of a block: ||G_ij - R_ij||_F / sqrt(||R_ii||_F ||R_jj||_F) (a cross block can be arbitrarily small: its own norm is no scale).
Limits: analytic 1e-8, the project's; numeric per pass 10x the largest error measured on an MI355X over that pass's cases here (DESIGN.md
§3 lists every case); a block is held to max(limit, KAPPA_EPS * kappa(H_kept)) as in the existing covariance files."""
import functools

import numpy as np
import pytest

from test_gpu_snapshot_covariance import KAPPA_EPS
import _general_cov_inputs as G
import _joint_cov_models as M
from _covariance_ref import hessian

pytestmark = pytest.mark.gpu

LOC_ERR_INVALID, LOC_ERR_UNSUPPORTED, LOC_ERR_SINGULAR = -1, -5, -6
I32_MIN = np.iinfo(np.int32).min
# numeric: 10x the largest error measured per pass on an MI355X (chain 8.92e-12: the 15-pose twist windows, kappa 7.3e5; forest 1.09e-12: the
# isolated-pose case; arrowhead 1.86e-12: (130, 4); envelope 8.36e-13: the mixed batch) — none above its pass's marginal limit (1.5e-9,
# 8.5e-11, 1.5e-9, 8.4e-12); DESIGN.md §3 lists every case
TOL = {"chain": {"analytic": 1e-8, "numeric": 8.9e-11}, "forest": {"analytic": 1e-8, "numeric": 1.1e-11},
       "arrow": {"analytic": 1e-8, "numeric": 1.9e-11}, "envelope": {"analytic": 1e-8, "numeric": 8.4e-12}}
MARGINAL_TOL = {"analytic": 1e-8, "numeric": 8.4e-12}   # test_gpu_general_covariance.TOL: the envelope pass's marginals of a joint call


def _head(la, wb, n):
    """the first n windows of a batch"""
    if wb.B <= n:
        return wb
    return wb.take(np.arange(n))


def _tables(wb, per_window, npm=None):
    """(pairs [B][npm][2] with the unused slots poisoned, counts [B]) from a list of pairs per window"""
    npm = max(len(p) for p in per_window) if npm is None else npm
    pairs = np.full((wb.B, max(npm, 1), 2), I32_MIN, dtype=np.int32)
    counts = np.array([len(p) for p in per_window], dtype=np.int32)
    for w, p in enumerate(per_window):
        if p:
            pairs[w, :len(p)] = p
    return pairs, counts


# ---- the cases: name -> (batch, anchors, solver keywords, options, pass, pairs per window, Jacobian modes) --------------------------------------
def _chain_pairs(wb, ragged=True):
    out = []
    for w in range(wb.B):
        nv = int(wb.counts[w, 0])
        if nv == 1:
            p = [(0, 0)]
        else:   # adjacent in both orders, the ends in both orders, (i, i), a duplicate, two more
            p = [(0, 1), (1, 0), (0, nv - 1), (nv - 1, 0), (nv // 2, nv // 2), (0, 1), (nv - 2, nv - 1), (nv // 2, nv - 1), (2 % nv, 4 % nv), (4 % nv, 2 % nv)]
        if ragged and w == 3: p = []
        if ragged and w == 5: p = p[:3]
        out.append(p)
    return out


def _forest_pairs(wb, deepest=False):
    out = []
    for w in range(wb.B):
        nv = int(wb.counts[w, 0])
        parent = M.forest_parents(nv, M.pose_pairs(wb, w))
        depth = [0] * nv
        for v in range(nv):
            u = v
            while parent[u] >= 0: u = parent[u]; depth[v] += 1
        root_of = list(range(nv))
        for v in sorted(range(nv), key=lambda v: depth[v]):
            if parent[v] >= 0: root_of[v] = root_of[parent[v]]
        leaves = [v for v in range(nv) if v not in parent and parent[v] >= 0]
        kids = {}
        for v in leaves: kids.setdefault(parent[v], []).append(v)
        keys = sorted(kids)
        p = [(leaves[0], parent[leaves[0]]), (parent[leaves[0]], leaves[0]), (3, 3), (0, nv - 1), (nv - 1, 0)]
        p += [(k[0], k[1]) for k in kids.values() if len(k) > 1][:2]                       # two leaves of one key
        if len(keys) > 1: p += [(kids[keys[0]][0], kids[keys[-1]][-1]), (kids[keys[-1]][-1], kids[keys[0]][0])]   # leaves of different keys
        other = [v for v in range(nv) if root_of[v] != root_of[0]]
        if other: p += [(0, other[-1]), (other[0], 1)]                                      # poses of different trees
        if deepest:
            by_depth = sorted(range(nv), key=lambda v: -depth[v])
            p += [(by_depth[0], by_depth[1]), (by_depth[0], root_of[by_depth[0]])]
        out.append(p)
    return out


def _arrow_pairs(wb):
    from _arrow_cov_inputs import ranged_nodes
    out = []
    for w in range(wb.B):
        nv = int(wb.counts[w, 0])
        nb = len(ranged_nodes(wb, w)[1])
        nc = nv - nb
        p = [(a, b) for a in range(nc, nv) for b in range(nc, nv)] if nb <= 6 else [(a, b) for a in range(nc, nv) for b in range(a, nv)]
        p += [(0, nc), (nv - 1, nc - 1), (nc // 2, nv - 1), (0, 1), (1, 0), (0, nc - 1), (nc - 1, 0), (nc // 2, nc // 2), (nc - 1, 1), (0, 1)]
        out.append(p)
    return out


def _outside_pairs(wb, extra):
    """per window: a pair outside its original envelope (where one exists: the key-first star's is full), one inside, a diagonal, and extra(nv)"""
    out = []
    for w in range(wb.B):
        nv = int(wb.counts[w, 0])
        first = G.envelope_first(nv, G.window_pairs(wb, w))
        outside = [(i, j) for i in range(nv) for j in range(i) if j < first[i]]
        p = [(0, 1), (1, 0), (nv - 1, nv - 1)] + extra(nv)
        if outside: p += [outside[0], outside[-1], outside[-1][::-1], outside[len(outside) // 2]]
        out.append(p)
    return out


def _case(la, name):
    from test_gpu_covariance import _observable_batch, _twist_batch
    from test_gpu_window_parity import ANCH
    both = ("analytic", "numeric")
    if name.startswith("chain3_"):
        T = int(name[7:])
        wb = _observable_batch(la, np.random.default_rng(700 + T), 8, T, False, False, translation_only=True)
        return wb, ANCH, {}, {}, "chain", _chain_pairs(wb), both
    if name == "chain6_imu_lever_12":
        wb = _observable_batch(la, np.random.default_rng(712), 8, 12, True, True)
        return wb, ANCH, {}, {}, "chain", _chain_pairs(wb), both
    if name == "chain6_twist_15":
        wb = _twist_batch(la, np.random.default_rng(715), 8, 15, True)
        return wb, ANCH, {}, {}, "chain", _chain_pairs(wb), both
    if name == "chain6_rotation_excluded":   # no lever arm, the IMU priors of every third pose dropped: those rotations are excluded
        wb = _observable_batch(la, np.random.default_rng(77), 8, 12, True, False)
        for i in range(wb.B):
            keep = [e for e in range(int(wb.counts[i, 2])) if wb.p_idx[i, e] % 3 != 1]
            wb.p_idx[i, :len(keep)] = wb.p_idx[i, keep].copy(); wb.p_val[i, :len(keep)] = wb.p_val[i, keep].copy()
            wb.counts[i, 2] = len(keep)
        return wb, ANCH, {}, {}, "chain", _chain_pairs(wb), ("numeric",)
    if name.startswith("forest_"):
        from test_gpu_forest_covariance import ANCH as FANCH, _case as forest_case
        wb = _head(la, forest_case(la, name[7:])[0], 8)
        # (rich_10_1, every pose a key, is a chain of EdgeSE3 with a gap: covariance_kind tests chains first, so the chain pass serves it)
        pass_ = "chain" if name == "forest_rich_10_1" else "forest"
        return wb, FANCH, {"bw_max": wb.caps[0] - 1, "chain_threshold": 1}, {}, pass_, _forest_pairs(wb, deepest=name == "forest_random_64"), both
    if name.startswith("arrow_"):
        from _arrow_cov_inputs import CASES, SURVEYED, case_batch
        wb = case_batch(la, name[6:])
        opt = {} if CASES[name[6:]][3] is None else {"arrow3": CASES[name[6:]][3]}
        return wb, SURVEYED, {}, opt, "arrow", _arrow_pairs(wb), CASES[name[6:]][4]
    gen = {"covariance_general": 1}
    if name == "env_mixed":
        wb = G.mixed_batch(la)
        return wb, G.ANCH, {}, gen, "envelope", _outside_pairs(wb, lambda nv: [(0, nv - 1)]), both
    if name == "env_chain3_65":
        wb = G.case_batch(la, "chain3_65")
        return wb, G.ANCH, {}, gen, "envelope", _outside_pairs(wb, lambda nv: [(0, nv - 1), (nv - 1, 0)]), both
    if name == "env_tall_stars":
        wb = G.case_batch(la, "tall_stars")
        return wb, G.ANCH, {}, gen, "envelope", _outside_pairs(wb, lambda nv: [(0, nv - 1), (5, 60), (60, 5)]), both
    if name == "env_keyframe_300":
        wb = G.case_batch(la, "keyframe_300")
        return wb, G.ANCH, {}, gen, "envelope", _outside_pairs(wb, lambda nv: [(299, 150), (150, 299)]), ("numeric",)
    raise KeyError(name)


CASES = ["chain3_1", "chain3_2", "chain3_10", "chain3_64", "chain6_imu_lever_12", "chain6_twist_15", "chain6_rotation_excluded",
         "forest_rich_10_1", "forest_rich_24_4", "forest_isolated_pose", "forest_random_64", "forest_doubled_se3",
         "arrow_5_1", "arrow_24_4", "arrow_70_6", "arrow_130_4",
         "env_mixed", "env_chain3_65", "env_tall_stars", "env_keyframe_300"]


def _solver(la, case, jac, general=None):
    wb, anchors, kw, opt = case[:4]
    s = la.WindowSolver(anchors, wb.B, *wb.caps, jacobian=jac, **kw)
    for k, v in opt.items():
        s.set_option(k, v)
    return s


@functools.lru_cache(maxsize=None)
def _solved(name, jac):
    """(case at the GPU's poses, the joint call's outputs, the plain call's, the pair tables); shared, never modified"""
    import localization_amd as la
    case = _case(la, name)
    wb = case[0]
    s = _solver(la, case, jac)
    s.solve(wb)
    pairs, counts = _tables(wb, case[5])
    plain = s.covariance(wb)
    joint = s.joint_covariance(wb, pairs, counts)
    assert s.last_covariance_ms() > 0
    s.close()
    return case, joint, plain, (pairs, counts)


def _check(case, jac, joint, plain, tables, label):
    """every requested block of every window against the reference, and the properties of DESIGN.md §2"""
    from oracle import oracle as O
    wb, anchors, _, _, pass_, per_window, _ = case
    cov, mask, status, cross = joint
    pairs, counts = tables
    mode = O.JAC_ANALYTIC if jac == "analytic" else O.JAC_NUMERIC_G2O
    worst, kmax = 0.0, 0.0
    assert not status.any()
    if pass_ == "envelope":
        assert np.array_equal(mask, plain[1]) and np.array_equal(status, plain[2])
    else:   # the three structured passes: the marginals of a joint call are bitwise those of the plain call
        assert all(np.array_equal(x, y) for x, y in zip((cov, mask, status), plain))
    for w in range(wb.B):
        nv, n = int(wb.counts[w, 0]), int(counts[w])
        assert not cross[w, n:].any()                                   # slots >= pair_counts are 0
        H = hessian(wb, w, anchors, mode)
        Sig, keep = M.kept_inverse(H)
        kappa = np.linalg.cond(H[np.ix_(keep, keep)])
        kmax = max(kmax, kappa)
        tol = max(TOL[pass_][jac], KAPPA_EPS * kappa)
        if pass_ == "envelope":   # the added blocks change the order of no sum: the marginals meet the general file's tolerance
            mtol = max(MARGINAL_TOL[jac], KAPPA_EPS * kappa)
            for v in range(nv):
                r = M.blk(Sig, v, v)
                assert np.linalg.norm(cov[w, v] - r) <= mtol * np.linalg.norm(r), (label, w, v)
        seen = {}
        for p in range(n):
            i, j = int(pairs[w, p, 0]), int(pairs[w, p, 1])
            g = cross[w, p]
            err = M.block_error(g, Sig, i, j)
            worst = max(worst, err)
            assert err <= tol, (label, w, (i, j), err, tol, kappa)
            for k in range(6):                                          # excluded rows of pose i, excluded columns of pose j
                if (mask[w, i] >> k) & 1: assert not g[k].any()
                if (mask[w, j] >> k) & 1: assert not g[:, k].any()
            if pass_ in ("arrow",) or label.startswith("chain3"):
                assert not g[3:].any() and not g[:, 3:].any()
            if i == j:
                assert np.array_equal(g, cov[w, i])                     # (i, i) has the bits of cov[i]
            if (i, j) in seen: assert np.array_equal(g, seen[(i, j)])   # duplicates return equal bits
            if (j, i) in seen: assert np.array_equal(g, seen[(j, i)].T) # (j, i) is bitwise the transpose of (i, j)
            seen[(i, j)] = g
            if not M.blk(Sig, i, j).any():                              # poses nothing connects: exact zeros on the GPU
                assert not g.any()
            ki, kj = ~((mask[w, i] >> np.arange(6)) & 1).astype(bool), ~((mask[w, j] >> np.arange(6)) & 1).astype(bool)
            J = np.block([[cov[w, i][np.ix_(ki, ki)], g[np.ix_(ki, kj)]], [g[np.ix_(ki, kj)].T, cov[w, j][np.ix_(kj, kj)]]])
            ev = np.linalg.eigvalsh((J + J.T) / 2)
            assert ev.min() >= -1e-12 * ev.max(), (label, w, (i, j), ev.min(), ev.max())
    print(f"joint covariance {label} {jac}: max block error {worst:.3e}, limit {TOL[pass_][jac]:.1e}, largest kappa {kmax:.3e}")
    return worst


PARITY = [(name, jac) for name in CASES for jac in ("analytic", "numeric")
          if not (jac == "analytic" and name in ("chain6_rotation_excluded", "arrow_70_6", "arrow_130_4", "env_keyframe_300")) and
          not (jac == "numeric" and name == "arrow_5_1")]


@pytest.mark.parametrize("name,jac", PARITY)
def test_parity_with_the_reference(gpu, name, jac):
    case, joint, plain, tables = _solved(name, jac)
    assert jac in case[6]
    _check(case, jac, joint, plain, tables, name)
    wb, (cov, mask, status, cross) = case[0], joint
    pairs, counts = tables
    if name == "chain3_1":
        assert (wb.counts[:, 0] == 1).all() and all(p in ([], [(0, 0)]) for p in case[5])
    if name.startswith("chain3_") and wb.caps[0] >= 10:
        # window 2 misses the link 2 - 3: two independent chains, exact zeros between them
        p = case[5][2].index((0, int(wb.counts[2, 0]) - 1))
        assert not cross[2, p].any() and cross[2, 0].any()
    if name == "chain6_rotation_excluded":
        assert (mask[:, 1] == 0x38).all() and not mask[:, 0].any()
        assert not cross[0, 0][:, 3:].any() and cross[0, 0][:3, :3].all()      # pair (0, 1): pose 1's rotation columns are 0
    if name == "forest_rich_24_4":
        assert any(not cross[0, p].any() for p in range(counts[0]))            # poses of different trees
    if name == "forest_isolated_pose":
        T = wb.caps[0]
        p = case[5][0].index((0, T - 1))
        assert not cross[:, p].any()


def test_the_forest_cases_run_both_solve_kernels(gpu):
    import localization_amd as la
    for name, kernel in (("forest_rich_24_4", "tree_wave_kernel"), ("forest_doubled_se3", "tree_lm_kernel")):
        case = _case(la, name)
        s = _solver(la, case, "numeric")
        s.solve(case[0])
        assert s.last_kernel_kind() == kernel
        s.close()


@pytest.mark.parametrize("jac", ["analytic", "numeric"])
def test_envelope_pass_agrees_with_the_chain_pass(gpu, jac):
    """The same twelve-pose 6-DoF chains on a 64-slot handle (covariance_kernel<6>) and on a 65-slot handle (the envelope pass)"""
    import localization_amd as la
    out = {}
    poses = None
    for nv_max in (64, 65):
        wb = G.chain_batch(la, 9301, 8, 12, True, nv_max=nv_max)
        s = la.WindowSolver(G.ANCH, wb.B, *wb.caps, jacobian=jac)
        s.set_option("covariance_general", 1)
        if poses is None:
            s.solve(wb)
            poses = wb.poses.copy()
        else:
            wb.poses[:, :64] = poses
        pairs, counts = _tables(wb, _chain_pairs(wb, ragged=False))
        out[nv_max] = (wb, s.joint_covariance(wb, pairs, counts), pairs, counts)
        s.close()
    (wa, ja, pairs, counts), (wc, jc, _, _) = out[65], out[64]
    assert not ja[2].any() and not jc[2].any()
    worst = 0.0
    for w in range(wa.B):
        for p in range(int(counts[w])):
            i, j = pairs[w, p]
            scale = np.sqrt(np.linalg.norm(jc[0][w, i]) * np.linalg.norm(jc[0][w, j]))
            worst = max(worst, np.linalg.norm(ja[3][w, p] - jc[3][w, p]) / scale)
    print(f"joint covariance, envelope pass against covariance_kernel<6> {jac}: max block difference {worst:.3e}")
    assert worst <= TOL["envelope"][jac]


# ---- isolation -----------------------------------------------------------------------------------------------------------------------------------
def _singular_case(la, pass_):
    """(good batch, bad batch, the singular window, anchors, solver keywords, options) by the existing files' constructions"""
    from oracle import oracle as O
    if pass_ == "chain":      # a window whose only pose is joined to nothing but one range with a lever arm (rank-1 H)
        from test_gpu_covariance import _observable_batch
        from test_gpu_window_parity import ANCH
        wb = _observable_batch(la, np.random.default_rng(11), 8, 12, True, True)
        bad, i = wb.copy(), 4
        bad.counts[i] = (1, 1, 0, 0)
        bad.r_idx[i, 0] = (0, -1 - 1); bad.r_val[i, 0] = (3.0, 100.0, 0.1, 0.0, -0.05)
        return wb, bad, i, ANCH, {}, {}
    if pass_ == "forest":     # one window loses the information of all its range edges: a gauge-free tree
        from test_gpu_tree_parity import ANCH, _forest_batch
        wb = _forest_batch(la, np.random.default_rng(8300), 8, 24, 4, False)
        bad, i = wb.copy(), 4
        bad.r_val[i, :, 1] = 0.0
        return wb, bad, i, ANCH, {"bw_max": 23, "chain_threshold": 1}, {}
    if pass_ == "arrow":      # one window loses its anchor priors and its ranges to surveyed anchors
        from _arrow_cov_inputs import SURVEYED, arrow_cov_batch, cut_gauge
        wb = arrow_cov_batch(la, np.random.default_rng(9300), 5, 24, 4, False)
        bad, i = wb.copy(), 2
        cut_gauge(bad, i)
        return wb, bad, i, SURVEYED, {}, {"arrow3": 1}
    wb = G.mixed_batch(la)    # the leaves-first star loses every range
    bad, i = wb.copy(), G.MIXED_STAR
    bad.counts[i, 1] = 0
    assert G.min_relative_pivot(hessian(bad, i, G.ANCH, O.JAC_NUMERIC_G2O)) < 1e-12
    return wb, bad, i, G.ANCH, {}, {"covariance_general": 1}


@pytest.mark.parametrize("pass_", ["chain", "forest", "arrow", "envelope"])
def test_singular_window_is_isolated(gpu, pass_):
    """A singular window has NaN in its requested cross blocks (0 in its unused slots); its neighbours' bits equal those of the batch without it."""
    import localization_amd as la
    wb, bad, i, anchors, kw, opt = _singular_case(la, pass_)
    s = _solver(la, (wb, anchors, kw, opt), "numeric")
    s.solve(wb)
    bad.poses[:] = wb.poses
    per_window = []
    for w in range(wb.B):
        nv = int(min(wb.counts[w, 0], bad.counts[w, 0]))
        per_window.append([(0, 0), (0, 0)] if w == i else [(0, nv - 1), (nv - 1, 0), (1, 1), (nv // 2, 0)])
    pairs, counts = _tables(wb, per_window)
    good = s.joint_covariance(wb, pairs, counts)
    assert not good[2].any() and np.isfinite(good[3]).all()
    got = s.joint_covariance(bad, pairs, counts)
    s.close()
    assert got[2][i] == LOC_ERR_SINGULAR and np.isnan(got[3][i, :2]).all() and not got[3][i, 2:].any()
    others = [k for k in range(wb.B) if k != i]
    assert (got[2][others] == 0).all()
    assert all(np.array_equal(x[others], y[others]) for x, y in zip(got, good))


# ---- resident = host ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["chain6_twist_15", "forest_rich_24_4", "arrow_24_4", "env_mixed"])
def test_resident_matches_host_bit_for_bit(gpu, name):
    """joint_covariance_resident = joint_covariance(wb) at the downloaded poses: right after the solve, with no solve in between (and other
    pairs), after another solve, and on a second stream; the solves equal those of a handle that never makes a joint call."""
    import torch
    import localization_amd as la
    case = _case(la, name)
    wb = case[0]
    B, T = wb.B, wb.caps[0]
    a, b = _solver(la, case, "numeric"), _solver(la, case, "numeric")
    wa, wc = wb.copy(), wb.copy()
    a.upload(wa); b.upload(wc)
    a.solve_resident(); b.solve_resident()
    pairs, counts = _tables(wb, case[5])
    npm = pairs.shape[1]
    fewer = np.minimum(counts, 2).astype(np.int32)

    def fresh():
        return (torch.full((B, T, 6, 6), 7.0, dtype=torch.float64, device=gpu), torch.full((B, T), 7, dtype=torch.int32, device=gpu),
                torch.full((B,), 7, dtype=torch.int32, device=gpu), torch.full((B, npm, 6, 6), 7.0, dtype=torch.float64, device=gpu))

    outs = [fresh() for _ in range(4)]
    a.joint_covariance_resident(pairs, counts, *outs[0])
    assert a.last_covariance_ms() > 0
    volatile_pairs, volatile_counts = pairs.copy(), fewer.copy()
    a.joint_covariance_resident(volatile_pairs, volatile_counts, *outs[1])      # no solve in between, other counts
    volatile_pairs[:] = I32_MIN; volatile_counts[:] = 99                         # (the caller's arrays are not read after the call returns)
    a.solve_resident(); b.solve_resident()
    a.joint_covariance_resident(pairs, counts, *outs[2])                         # a solve in between
    other = torch.cuda.Stream(device=gpu)
    torch.cuda.synchronize()
    a.joint_covariance_resident(pairs, counts, *outs[3], stream=other)
    other.synchronize()
    plain_d = fresh()[:3]
    a.covariance_resident(*plain_d)                                              # the plain call on the same handle: the joint call without pairs
    ra, rb = a.download(wa).copy(), b.download(wc).copy()
    used = np.arange(T)[None, :] < wa.counts[:, :1]
    assert np.array_equal(wa.poses[used], wc.poses[used]) and np.array_equal(ra, rb) and a.last_kernel_kind() == b.last_kernel_kind()
    host = a.joint_covariance(wa, pairs, counts)
    host_fewer = a.joint_covariance(wa, pairs, fewer)
    assert not host[2].any()
    for k, want in ((0, host), (1, host_fewer), (2, host), (3, host)):
        assert all(np.array_equal(t.cpu().numpy(), h) for t, h in zip(outs[k], want)), k
    assert all(np.array_equal(t.cpu().numpy(), h) for t, h in zip(plain_d, a.covariance(wa)))
    # host-path joint calls between host solves leave those alone as well
    w1, w2 = wb.copy(), wb.copy()
    r1 = a.solve(w1).copy(); a.joint_covariance(w1, pairs, counts); r1b = a.solve(wb.copy()).copy()
    r2 = b.solve(w2).copy()
    assert np.array_equal(w1.poses[used], w2.poses[used]) and np.array_equal(r1, r2) and np.array_equal(r1b, r2)
    a.close(); b.close()


def test_resident_pair_table_grows_and_is_kept(gpu):
    """One handle, three windows of four poses, resident joint calls with npair_max = 1, then 3 (the pair table grows), then 1 (the larger
    table is kept): each has the bits of a fresh handle's only call."""
    import torch
    import localization_amd as la
    from test_gpu_covariance import _observable_batch
    from test_gpu_window_parity import ANCH
    wb = _observable_batch(la, np.random.default_rng(733), 3, 4, False, False, translation_only=True)
    B, T = wb.B, wb.caps[0]
    per_window = {1: [[(0, 1)], [(1, 0)], [(3, 0)]], 3: [[(1, 0), (0, 0), (0, 1)], [(0, 3), (2, 1)], [(3, 3), (1, 2), (2, 0)]]}

    def ready():
        s = la.WindowSolver(ANCH, B, *wb.caps, jacobian="numeric")
        s.upload(wb.copy()); s.solve_resident()
        return s

    def call(s, npm):
        pairs, counts = _tables(wb, per_window[npm], npm=npm)
        out = (torch.full((B, T, 36), 7.0, dtype=torch.float64, device=gpu), torch.full((B, T), 7, dtype=torch.int32, device=gpu),
               torch.full((B,), 7, dtype=torch.int32, device=gpu), torch.full((B, npm, 36), 7.0, dtype=torch.float64, device=gpu))
        torch.cuda.synchronize()
        s.joint_covariance_resident(pairs, counts, *out)
        torch.cuda.synchronize()
        return tuple(t.cpu().numpy() for t in out)

    one = ready()
    got = [call(one, npm) for npm in (1, 3, 1)]
    one.close()
    for k, npm in enumerate((1, 3, 1)):
        fresh = ready()
        want = call(fresh, npm)
        fresh.close()
        assert not want[2].any() and np.isfinite(want[3]).all() and want[3][0, 0].any()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got[k], want)), (k, npm)


# ---- refusals write nothing -----------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(gpu):
    import torch
    import localization_amd as la
    from test_gpu_chain3_parity import _translation_only_batch
    case = _case(la, "chain3_10")
    wb = case[0]
    B, T = wb.B, wb.caps[0]
    s = _solver(la, case, "numeric")
    s.solve(wb)
    s.upload(wb); s.solve_resident()
    ok_pairs, ok_counts = _tables(wb, [[(0, 0), (0, 1)]] * B, npm=3)
    s.joint_covariance(wb, ok_pairs, ok_counts)

    def refused(batch, pairs, counts, code, resident=True, handle=s):
        npm = pairs.shape[1]
        out = (np.full((batch.B, T, 6, 6), 7.0), np.full((batch.B, T), 7, dtype=np.int32), np.full(batch.B, 7, dtype=np.int32), np.full((batch.B, npm, 6, 6), 7.0))
        with pytest.raises(la.LocalizationAmdError) as ex:
            handle.joint_covariance(batch, pairs, counts, out=out)
        assert ex.value.code == code
        assert all((o == 7).all() for o in out)
        if not resident:
            return
        dev = tuple(torch.full(o.shape, 7, dtype=torch.float64 if o.dtype == np.float64 else torch.int32, device=gpu) for o in out)
        torch.cuda.synchronize()
        with pytest.raises(la.LocalizationAmdError) as ex:
            handle.joint_covariance_resident(pairs, counts, *dev)
        assert ex.value.code == code
        torch.cuda.synchronize()
        assert all((t == 7).all().item() for t in dev)

    nv0 = int(wb.counts[0, 0])                                  # window 0 is a short one: a slot that exists in its neighbours
    assert nv0 < T
    bad = ok_pairs.copy(); bad[0, 1, 1] = nv0
    refused(wb, bad, ok_counts, LOC_ERR_INVALID)                # a pair slot >= nv
    bad = ok_pairs.copy(); bad[B - 1, 0, 0] = -1
    refused(wb, bad, ok_counts, LOC_ERR_INVALID)                # a negative slot
    bad = ok_counts.copy(); bad[3] = 4
    refused(wb, ok_pairs, bad, LOC_ERR_INVALID)                 # pair_counts > npair_max
    bad = ok_counts.copy(); bad[3] = -1
    refused(wb, ok_pairs, bad, LOC_ERR_INVALID)
    s.close()
    # an unsupported batch: chains of 65 poses on a handle without option "covariance_general"
    long = _translation_only_batch(la, np.random.default_rng(5), 2, 65, False)
    T = 65
    h = la.WindowSolver(case[1], 2, *long.caps)
    h.upload(long); h.solve_resident()
    p, c = _tables(long, [[(0, 1), (1, 0)]] * 2)
    refused(long, p, c, LOC_ERR_UNSUPPORTED, handle=h)
    h.close()


def test_no_pairs_is_the_plain_call(gpu):
    """npair_max = 0 is valid: cov, mask and status of the plain call"""
    case, joint, plain, _ = _solved("chain6_twist_15", "numeric")
    import localization_amd as la
    s = _solver(la, case, "numeric")
    got = s.joint_covariance(case[0], np.zeros((case[0].B, 0, 2), dtype=np.int32))
    s.close()
    assert got[3].size == 0 and all(np.array_equal(x, y) for x, y in zip(got[:3], plain))
