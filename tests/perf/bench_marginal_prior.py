#!/usr/bin/env python3
"""Time per launch of the marginal-prior pass (loc_window_marginal_prior_host: marginal_prior_kernel) next to the plain covariance call
(loc_window_covariance_host: covariance_kernel<3>) and the solve of the SAME batch in the same run: 65 536 translation-only chains of ten
poses with four anchors each (tests/_fixed_lag.py), the oldest pose dropped.  Then the general kernel on one batch with and without a table
of full information matrices holding the same values (diag(p_val's diagonal)): 4 096 of those chains with a position prior on every pose,
the handle kept on window_lm_kernel by chain threshold 0.  HIP events around the launches (loc_window_last_covariance_ms /
loc_window_last_kernel_ms), alternated, median and best of --reps.  Prints one JSON line per row.

    python tests/perf/bench_marginal_prior.py [--reps 7] [--windows 65536] [--jacobian numeric]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _row(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "best_ms": round(min(ms), 4), "spread": round(max(ms) / min(ms) - 1, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--windows", type=int, default=65536)
    ap.add_argument("--jacobian", default="numeric")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.append(os.path.join(ROOT, "tests"))
    import localization_amd as la
    import _fixed_lag as F
    T, distinct = 10, 256
    small = la.WindowBatch(distinct, T, T * 4 + (T - 1), 0, 0)
    for i in range(distinct):
        F.add_chain_poses(small, i, F.Chain(100 + i, T, 4), 0, T)
    wb = small.tile(args.windows)
    s = la.WindowSolver(F.ANCH, wb.B, *wb.caps, jacobian=args.jacobian, bw_max=1)
    s.solve(wb)   # (the passes below run at the solved estimates)
    solve_kernel = s.last_kernel_kind()
    drop = np.zeros(wb.B, dtype=np.int32)
    mp_out, cov_out = None, None
    ms = {"marginal": [], "covariance": [], "solve": []}
    start = wb.poses.copy()
    for rep in range(args.reps + 1):
        mp_out = s.marginal_prior(wb, drop, out=mp_out)
        t_mp = s.last_covariance_ms()
        cov_out = s.covariance(wb, out=cov_out)
        t_cov = s.last_covariance_ms()
        again = wb.tile(wb.B) if rep == 0 else again
        again.poses[:] = start
        s.solve(again)
        if rep:   # (the first round allocates)
            ms["marginal"].append(t_mp); ms["covariance"].append(t_cov); ms["solve"].append(s.last_kernel_ms())
    shape = f"{wb.B} translation-only chains x T = 10, 4 anchors per pose, {args.jacobian} Jacobians"
    print(json.dumps({"pass": "marginal_prior_kernel", "shape": shape, **_row(ms["marginal"]), "rank_1_windows": int((mp_out[4] == 1).sum()),
                      "singular_windows": int((mp_out[5] != 0).sum())}), flush=True)
    print(json.dumps({"pass": "covariance_kernel<3>", "shape": shape, **_row(ms["covariance"]), "singular_windows": int((cov_out[2] != 0).sum())}), flush=True)
    print(json.dumps({"pass": solve_kernel, "shape": shape, **_row(ms["solve"])}), flush=True)
    print(json.dumps({"marginal_over_covariance": round(float(np.median(ms["marginal"]) / np.median(ms["covariance"])), 3),
                      "marginal_over_solve": round(float(np.median(ms["marginal"]) / np.median(ms["solve"])), 3)}), flush=True)
    s.close()

    # ---- the general kernel with and without the table, the same values ------------------------------------------------------------------------
    B = min(4096, args.windows)
    small = la.WindowBatch(distinct, T, T * 4 + (T - 1), T, 0)
    for i in range(distinct):
        ch = F.Chain(100 + i, T, 4)
        F.add_chain_poses(small, i, ch, 0, T)
        for k in range(T):
            small.add_prior(i, k, ch.est[k], np.eye(3), np.array([25.0, 25.0, 25.0, 0, 0, 0]))
    base = small.tile(B)
    s = la.WindowSolver(F.ANCH, B, *base.caps, jacobian=args.jacobian, bw_max=1, chain_threshold=0)
    work = base.tile(B)
    table = np.zeros((B, T, 36))
    table[:, :, ::7] = base.p_val[:, :, 12:]
    ms = {False: [], True: []}
    poses = {}
    for rep in range(args.reps + 1):
        for with_table in (False, True):
            work.poses[:] = base.poses
            work.p_info = table if with_table else None
            s.solve(work)
            assert s.last_kernel_kind() == "window_lm_kernel"
            poses[with_table] = work.poses.copy()
            if rep:
                ms[with_table].append(s.last_kernel_ms())
    shape = f"{B} translation-only chains x T = 10 with a position prior per pose, {args.jacobian} Jacobians"
    print(json.dumps({"pass": "window_lm_kernel", "priors": "diagonal (p_val)", "shape": shape, **_row(ms[False])}), flush=True)
    print(json.dumps({"pass": "window_lm_kernel<PINFO>", "priors": "table of full matrices, the same values", "shape": shape, **_row(ms[True]),
                      "over_diagonal": round(float(np.median(ms[True]) / np.median(ms[False])), 3),
                      "largest_pose_difference_m": float(np.abs(poses[True] - poses[False]).max())}), flush=True)
    s.close()


if __name__ == "__main__":
    main()
