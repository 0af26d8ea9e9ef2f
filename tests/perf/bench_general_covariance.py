#!/usr/bin/env python3
"""Throughput of the envelope covariance pass (envelope_covariance_kernel.hip, option "covariance_general") next to the solve of the same
device-resident batch, numeric Jacobians, at two shapes:
  (a) 4 096 translation-only chains x 128 poses (every pose ranged to all four anchors) — and, for scale, covariance_kernel<3> on the
      64-pose version of the same windows;
  (b) 64 key-frame windows x 500 poses of cfg/uwb_pose.yaml's topology (a key every 10 poses), packed leaves-first.
Both timed with HIP events around the launches (loc_window_timing_* for the solve, loc_window_last_covariance_ms for the covariance), best
of --reps.  Prints one JSON line per shape.

    python tests/perf/bench_general_covariance.py [--reps 5] [--shape a|b|all]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _run(la, torch, wb, reps, general):
    from _general_cov_inputs import ANCH
    B, T = wb.B, wb.caps[0]
    s = la.WindowSolver(ANCH, B, *wb.caps, jacobian="numeric")
    s.set_option("covariance_general", int(general))
    s.upload(wb)
    s.solve_resident()
    cov = torch.empty((B, T, 36), dtype=torch.float64, device="cuda")
    mask = torch.empty((B, T), dtype=torch.int32, device="cuda")
    status = torch.empty((B,), dtype=torch.int32, device="cuda")
    solve_ms, cov_ms, kind = [], [], None
    for _ in range(reps):
        s.timing_begin(1)
        s.solve_resident()
        _, tot, _ = s.timing_end()
        solve_ms.append(tot)
        kind = s.last_kernel_kind()
        s.covariance_resident(cov, mask, status)
        cov_ms.append(s.last_covariance_ms())
    torch.cuda.synchronize()
    blocks, nbytes = s.covariance_plan(wb)
    singular = int((status.cpu() != 0).sum())
    s.close()
    return {"windows": B, "poses": T, "solve_kernel": kind, "solve_ms": round(min(solve_ms), 4), "covariance_ms": round(min(cov_ms), 4),
            "covariance_windows_per_s": round(B / min(cov_ms) * 1e3), "covariance_over_solve_time": round(min(cov_ms) / min(solve_ms), 2),
            "singular_windows": singular, "envelope_blocks_max": blocks, "envelope_workspace_MiB": round(nbytes / 2 ** 20, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shape", default="all")
    ap.add_argument("--batch-a", type=int, default=4096)
    ap.add_argument("--batch-b", type=int, default=64)
    args = ap.parse_args()
    import torch
    import localization_amd as la
    import _general_cov_inputs as G
    if args.shape in ("a", "all"):
        wb = G.chain_batch(la, 1, 64, 128, False, ragged=False).tile(args.batch_a)
        out = {"shape": "a: translation-only chains x 128 poses", "pass": "envelope_covariance_kernel", **_run(la, torch, wb, args.reps, True)}
        print(json.dumps(out), flush=True)
        wb = G.chain_batch(la, 1, 64, 64, False, ragged=False).tile(args.batch_a)
        out = {"shape": "a (scale): the same chains x 64 poses", "pass": "covariance_kernel<3>", **_run(la, torch, wb, args.reps, False)}
        print(json.dumps(out), flush=True)
    if args.shape in ("b", "all"):
        wb = G.keyframe_batch(la, 2, 8, 500, 10).tile(args.batch_b)
        out = {"shape": "b: key-frame windows x 500 poses, a key every 10, leaves-first", "pass": "envelope_covariance_kernel", **_run(la, torch, wb, args.reps, True)}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
