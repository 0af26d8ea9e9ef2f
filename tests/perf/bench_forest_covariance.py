#!/usr/bin/env python3
"""Throughput of the forest covariance pass (forest_covariance_kernel.hip) next to the solve of the same device-resident batch:
BASELINE config 5's shape, 16 384 windows x 64 poses (key-frame EdgeSE3 stars, a new key every 8 poses, one anchor range per pose),
numeric Jacobians.  Both timed with HIP events around the launches (loc_window_timing_* for the solve — tree_wave_kernel —,
loc_window_last_covariance_ms for the covariance), best of --reps.  Prints one JSON line.

    python tests/perf/bench_forest_covariance.py [--batch 16384] [--reps 5]
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
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    import localization_amd as la
    from test_gpu_tree_parity import ANCH, _forest_batch
    T = 64
    wb = _forest_batch(la, np.random.default_rng(0), 256, T, 8, False).tile(args.batch)
    B = wb.B
    s = la.WindowSolver(ANCH, B, *wb.caps, jacobian="numeric", bw_max=T - 1)
    s.upload(wb)
    s.solve_resident()
    kind = None
    cov = torch.empty((B, T, 36), dtype=torch.float64, device="cuda")
    mask = torch.empty((B, T), dtype=torch.int32, device="cuda")
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
    print(json.dumps({"shape": "cfg5_T64_every8", "windows": B, "solve_kernel": kind, "solve_ms": round(sm, 4), "covariance_ms": round(cm, 4),
                      "solve_windows_per_s": round(B / sm * 1e3), "covariance_windows_per_s": round(B / cm * 1e3),
                      "covariance_over_solve_throughput": round(sm / cm, 2), "singular_windows": singular}), flush=True)
    s.close()


if __name__ == "__main__":
    main()
