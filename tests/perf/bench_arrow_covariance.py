#!/usr/bin/env python3
"""Time of the arrowhead covariance pass (arrow_covariance_kernel.hip) next to the solve of the same device-resident batch: BASELINE
config 4's shape, 1 024 hypotheses x (256 tag poses + 10 unknown anchors), tiled from 32 distinct ones (bench_window.build_selfcal), with
numeric and with analytic range Jacobians.  Both timed with HIP events around the launches (loc_window_timing_* for the solve —
arrow3_lm_kernel —, loc_window_last_covariance_ms for the covariance), best of --reps.  Prints one JSON line per Jacobian mode.

    python tests/perf/bench_arrow_covariance.py [--batch 1024] [--reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "perf"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    import localization_amd as la
    import bench_window as bw
    B, nd = args.batch, 32
    small, _, anchors, nv = bw.build_selfcal(nd, np.random.default_rng(21))
    wb = small.tile(B)
    cov = torch.empty((B, nv, 36), dtype=torch.float64, device="cuda")
    mask = torch.empty((B, nv), dtype=torch.int32, device="cuda")
    status = torch.empty((B,), dtype=torch.int32, device="cuda")
    for jac in ("numeric", "analytic"):
        s = la.WindowSolver(anchors, B, *wb.caps, maximum_iteration=10, bw_max=nv - 1, jacobian=jac)
        s.upload(wb)
        s.solve_resident()
        s.covariance_resident(cov, mask, status)   # (the first call allocates the workspace)
        kind = None
        solve_ms, cov_ms = [], []
        for _ in range(args.reps):
            s.timing_begin(1)
            s.solve_resident()
            _, tot, _ = s.timing_end()
            solve_ms.append(tot)
            kind = s.last_kernel_kind()
            s.covariance_resident(cov, mask, status)
            cov_ms.append(s.last_covariance_ms())
        torch.cuda.synchronize()
        singular = int((status.cpu() != 0).sum())
        sm, cm = min(solve_ms), min(cov_ms)
        print(json.dumps({"shape": "cfg4_T256_A10", "windows": B, "jacobian": jac, "solve_kernel": kind, "solve_ms": round(sm, 4),
                          "covariance_ms": round(cm, 4), "covariance_over_solve_time": round(cm / sm, 3), "singular_windows": singular}), flush=True)
        s.close()


if __name__ == "__main__":
    main()
