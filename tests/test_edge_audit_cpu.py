"""CPU-side checks of the edge audit and the outlier-range removal (loc_window_edge_chi2_*, loc_window_prune_resident; DESIGN.md §2, "Edge audit
and outlier removal"): the ABI surface, the reference helper of the GPU tests against a closed form and the oracle's own chi2, the margins of
the GPU prune tests' inputs by the reference alone, and what the rule buys — measured on the oracle before any kernel runs."""
import ctypes as C

import numpy as np
import pytest

import _fixed_lag as F
import _edge_audit_cases as K
import _edge_audit_ref as R
from _covariance_ref import reference_covariance
from _oracle_window import oracle_solve_instance

LOC_ERR_INVALID = -1


# ---- (a) the three entry points --------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_exported_and_refuse_a_null_handle(built):
    import localization_amd as la
    L = la.lib()
    for name in ("loc_window_edge_chi2_host", "loc_window_edge_chi2_resident", "loc_window_prune_resident"):
        assert hasattr(L, name), name
    assert L.loc_window_edge_chi2_host(None, 1, *([None] * 13)) == LOC_ERR_INVALID
    assert L.loc_window_edge_chi2_resident(None, None, None, None, None, None, None) == LOC_ERR_INVALID
    assert b"nothing uploaded" in L.loc_last_error()
    assert L.loc_window_prune_resident(None, None, 2.0, 100, None, None) == LOC_ERR_INVALID
    assert la.abi_version() == 4
    for name in ("edge_chi2", "edge_chi2_resident", "prune_resident"):
        assert callable(getattr(la.WindowSolver, name))


# ---- (b) the helper ----------------------------------------------------------------------------------------------------------------------------------
def test_helper_agrees_with_the_closed_form_and_the_oracles_chi2(built):
    import localization_amd as la
    wb, _ = K.prune_batch(la)
    for i in range(wb.B):
        r, p, s, total, active, oracle_total = R.window_chi2(wb, i, F.ANCH)
        nr = int(wb.counts[i, 1])
        assert len(r) == nr and len(p) == 0 and len(s) == 0
        for e in range(nr):
            v0, v1 = int(wb.r_idx[i, e, 0]), int(wb.r_idx[i, e, 1])
            t = wb.poses[i, v0, 9:]
            a = F.ANCH[-1 - v1] if v1 < 0 else wb.poses[i, v1, 9:]
            want = wb.r_val[i, e, 1] * (np.linalg.norm(t - a) - wb.r_val[i, e, 0]) ** 2
            assert abs(r[e] - want) <= 1e-12 * (1.0 + want), (i, e, r[e], want)
        assert abs(total - oracle_total) <= 1e-12 * (1.0 + total), (i, total, oracle_total)
        assert active == nr - (1 if i == 2 else 0)
    # a 6-DoF window with priors: the sum against the oracle's all-edges chi2 at unchanged poses
    wb6, anch, _, _ = K.audit_case(la, "chain6_12")
    r, p, s, total, active, oracle_total = R.window_chi2(wb6, 0, anch)
    assert len(p) == 12 and abs(total - oracle_total) <= 1e-12 * (1.0 + total) and active == int(wb6.counts[0, 1]) + 12


# ---- (c) the prune inputs, by the reference alone -------------------------------------------------------------------------------------------------------
def _oracle_solved(la, wb, anchors, iterations=10, poses=None):
    out = wb.copy()
    if poses is not None:
        out.poses[:] = poses
    for i in range(wb.B):
        nv = int(wb.counts[i, 0])
        out.poses[i, :nv] = oracle_solve_instance(out, i, anchors, iterations=iterations)[0]
    return out


def test_prune_inputs_satisfy_the_margins_by_the_reference(built):
    import localization_amd as la
    wb, planted = K.prune_batch(la)
    solved = _oracle_solved(la, wb, F.ANCH)
    r, _, _, _, active = R.batch_chi2(solved, F.ANCH)
    assert R.margin(solved, r, K.PRUNE_CHI2_MAX) > 1e-6
    assert active[0] == K.PRUNE_MIN_EDGES and active[1] == K.PRUNE_MIN_EDGES + 1 and active[2] == K.PRUNE_MIN_EDGES
    assert (active[3:] > K.PRUNE_MIN_EDGES).all()
    assert (r[:, :planted.shape[1]][planted] > K.PRUNE_CHI2_MAX).all() and planted[[0, 1]].any(axis=1).all()
    removed, n_removed = R.prune_flags(solved, r, active, K.PRUNE_CHI2_MAX, K.PRUNE_MIN_EDGES)
    assert n_removed[0] == 0 and n_removed[2] == 0                       # at the threshold: everything stays, the planted outliers too
    for i in (1, 4, 5, 6, 7):
        assert removed[i, :planted.shape[1]][planted[i]].all(), i       # above it: every planted outlier goes


# ---- (d) what the rule buys --------------------------------------------------------------------------------------------------------------------------
def what_the_rule_buys(la, B=8, iterations=F.PROPERTY_ITERATIONS):
    """Per window of K.prune_batch's kind (50 active rows, two or three of 40 anchor ranges displaced by 1.5 m): the largest distance of a pose
    to the solution of the SAME window without the displacement after (single solve, solve -> prune by the rule -> solve from there), and
    trace(Sigma_newest) of the reference covariance at each of the two and at the outlier-free solution; rows removed, rows planted, planted
    rows removed.  Oracle and numpy alone, converged solves (tests/_fixed_lag.PROPERTY_ITERATIONS)."""
    rows = []
    for i in range(B):
        ch = F.Chain(9900 + i, K.PRUNE_T, 4)
        clean = la.WindowBatch(1, *F.window_caps(K.PRUNE_T))
        F.add_chain_poses(clean, 0, ch, 0, K.PRUNE_T, doubled=(1,))
        dirty = clean.copy()
        anchor_rows = [e for e in range(int(clean.counts[0, 1])) if clean.r_idx[0, e, 1] < 0]
        picks = [anchor_rows[(5 + 7 * i) % 40], anchor_rows[-1 - (i % 3)]] + ([anchor_rows[11]] if i % 2 else [])
        for e in picks:
            dirty.r_val[0, e, 0] += K.DISPLACED
        x0 = _oracle_solved(la, clean, F.ANCH, iterations)
        x1 = _oracle_solved(la, dirty, F.ANCH, iterations)
        r, _, _, _, active = R.batch_chi2(x1, F.ANCH)
        removed, n_removed = R.prune_flags(x1, r, active, K.PRUNE_CHI2_MAX, K.PRUNE_MIN_EDGES)
        x2 = _oracle_solved(la, R.with_rows_zeroed(la, x1, removed), F.ANCH, iterations)
        dist = lambda x: float(np.linalg.norm(x.poses[0, :, 9:] - x0.poses[0, :, 9:], axis=1).max())
        tr = lambda x: float(np.trace(reference_covariance(x, 0, F.ANCH, 1)[0][-1][:3, :3]))
        rows.append((dist(x1), dist(x2), tr(x0), tr(x1), tr(x2), int(n_removed[0]), len(picks), int(removed[0, picks].sum())))
    return np.array(rows)


def test_what_the_rule_buys_on_the_oracle(built):
    """The figures DESIGN.md §2 carries, whatever they are (there: on these windows the rule buys nothing measurable — the Cauchy kernel has
    already taken a 50 sigma range down to 1 / 2500 of its weight, and chi2 > 2 also removes the ~16 % of good ranges beyond 1.41 sigma).
    Asserted is only what follows from the inputs: a range displaced by 50 sigma has chi2 far above 2 at any estimate within a metre of
    the truth, so every planted row is removed; the second solve stays finite."""
    import localization_amd as la
    rows = what_the_rule_buys(la)
    for k, row in enumerate(rows):
        print(f"window {k}: |x - x_clean| single {row[0]:.4f} m, pruned {row[1]:.4f} m; trace Sigma_newest clean {row[2]:.3e}, single {row[3]:.3e}, "
              f"pruned {row[4]:.3e} m^2; removed {int(row[5])} (planted {int(row[6])})")
    print("median", np.median(rows, axis=0)[:5], "mean", rows.mean(axis=0)[:5])
    assert np.isfinite(rows).all()
    assert (rows[:, 7] == rows[:, 6]).all() and (rows[:, 5] >= rows[:, 6]).all()
