#!/usr/bin/env python3
"""Throughput of the marginal-covariance pass (covariance_kernel.hip) next to the solve of the same device-resident batch: 65 536 windows of
cfg/uwb_only.yaml (T = 10, translation-only: 3x3 blocks), cfg/uwb_imu.yaml (T = 12, IMU priors + lever arm) and cfg/uwb_twist.yaml (T = 15,
EdgeSE3 between consecutive poses).  Both timed with HIP events around the launches (loc_window_timing_* for the solve,
loc_window_last_covariance_ms for the covariance), best of --reps.  Prints one JSON line per shape.

    python tests/perf/bench_covariance.py [--batch 65536] [--reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    import localization_amd as la
    from test_gpu_covariance import _observable_batch, _twist_batch
    from test_gpu_window_parity import ANCH
    rng = np.random.default_rng(0)
    # (the reference's streams range one anchor per pose: the undamped H of such a window is singular — DESIGN.md §2 —, so these shapes
    #  range every pose to all four anchors)
    shapes = {"cfg1_T10": lambda: _observable_batch(la, rng, 1024, 10, False, False, translation_only=True),
              "uwb_imu_T12": lambda: _observable_batch(la, rng, 1024, 12, True, True),
              "uwb_twist_T15": lambda: _twist_batch(la, rng, 1024, 15, True)}
    for name, make in shapes.items():
        wb = make().tile(args.batch)
        B = wb.B
        s = la.WindowSolver(ANCH, B, *wb.caps, jacobian="numeric")
        s.upload(wb)
        s.solve_resident()
        kind = None
        cov = torch.empty((B, wb.caps[0], 36), dtype=torch.float64, device="cuda")
        mask = torch.empty((B, wb.caps[0]), dtype=torch.int32, device="cuda")
        status = torch.empty((B,), dtype=torch.int32, device="cuda")
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
        print(json.dumps({"shape": name, "windows": B, "solve_kernel": kind, "solve_ms": round(sm, 4), "covariance_ms": round(cm, 4),
                          "solve_windows_per_s": round(B / sm * 1e3), "covariance_windows_per_s": round(B / cm * 1e3),
                          "covariance_over_solve_throughput": round(sm / cm, 2), "singular_windows": singular}), flush=True)
        s.close()


if __name__ == "__main__":
    main()
