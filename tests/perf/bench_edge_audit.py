#!/usr/bin/env python3
"""What the per-edge chi2 audit and the resident outlier-range removal cost (loc_window_edge_chi2_resident, loc_window_prune_resident; DESIGN.md
§2 / §4) beside the resident solve they follow, on two shapes:
  chains     65 536 translation-only chains of 10 poses, 4 anchors per pose (tests/_fixed_lag.py's windows, tiled)
  keyframes  64 key-frame windows of 500 poses (tests/_general_cov_inputs.keyframe_batch's stars, every 10th pose a key, tiled from 4)

Per shape, median of --reps with the spread (min .. max), HIP events around the launch:
  audit_ms   loc_window_edge_chi2_resident, every output requested           (loc_window_last_covariance_ms)
  prune_ms   loc_window_prune_resident(2.0, 0) on a freshly solved upload     (loc_window_last_covariance_ms)
  solve_ms   the resident solve of the same batch                             (loc_window_timing_*)
and the bytes each pass must move — the used rows of every table it reads, once, plus its outputs — with the rate that makes of the time.
Prints one JSON line per shape.

    python tests/perf/bench_edge_audit.py [--reps 7] [--chains 65536] [--keyframes 64]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))


def _stats(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4)}


def _bytes(wb):
    """(audit, prune): the used rows of the tables each pass reads, once, plus what it writes (every slot of its outputs)"""
    nv, nr, np_, ns = (int(x) for x in wb.counts.sum(axis=0))
    B = wb.B
    ranges = 16 * B + nv * 96 + nr * (8 + 40)
    audit = ranges + np_ * (4 + 144) + ns * (16 + 384) + B * (wb.caps[1] + wb.caps[2] + wb.caps[3]) * 8 + B * 12
    prune = ranges + B * wb.caps[1] * 4 + B * 4
    return audit, prune


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--keyframes", type=int, default=64)
    args = ap.parse_args()
    import torch
    import localization_amd as la
    import _fixed_lag as F
    import _general_cov_inputs as G
    dev = torch.device("cuda", 0)
    shapes = (("chains", lambda: F.first_window(la, [F.Chain(9950 + i, 10, 4) for i in range(8)], 10).tile(args.chains), F.ANCH, {}),
              ("keyframes", lambda: G.keyframe_batch(la, 9960, 4, 500, 10).tile(args.keyframes), G.ANCH, {"chain_min_batch": 1}))
    for name, build, anchors, opts in shapes:
        wb = build()
        B = wb.B
        s = la.WindowSolver(anchors, B, *wb.caps, jacobian="numeric")
        for k, v in opts.items():
            s.set_option(k, v)
        outs = tuple(torch.zeros((B, max(wb.caps[k], 1)), dtype=torch.float64, device=dev) for k in (1, 2, 3)) + \
            (torch.zeros(B, dtype=torch.float64, device=dev), torch.zeros(B, dtype=torch.int32, device=dev))
        removed, n_removed = torch.zeros((B, max(wb.caps[1], 1)), dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        t = {"audit_ms": [], "prune_ms": [], "solve_ms": []}
        for rep in range(args.reps + 1):   # (the first round warms up: allocations, the first launches)
            s.upload(wb)
            s.timing_begin(1)
            s.solve_resident()
            solve_ms = s.timing_end()[2]
            s.edge_chi2_resident(*outs)
            audit_ms = s.last_covariance_ms()
            s.prune_resident(2.0, 0, removed, n_removed)
            prune_ms = s.last_covariance_ms()
            if rep:
                t["audit_ms"].append(audit_ms); t["prune_ms"].append(prune_ms); t["solve_ms"].append(solve_ms)
        torch.cuda.synchronize()
        audit_b, prune_b = _bytes(wb)
        row = {"shape": name, "windows": B, "poses": int(wb.counts[0, 0]), "rows_per_window": int(wb.counts[0, 1:].sum()), "reps": args.reps,
               "solve_kernel": s.last_kernel_kind(), "rows_removed": int(n_removed.sum().item()), "active_edges": int(outs[4].sum().item())}
        row.update({k: _stats(v) for k, v in t.items()})
        row["audit_bytes"] = audit_b; row["prune_bytes"] = prune_b
        row["audit_GBps"] = round(audit_b / (row["audit_ms"]["median"] * 1e-3) / 1e9, 1)
        row["prune_GBps"] = round(prune_b / (row["prune_ms"]["median"] * 1e-3) / 1e9, 1)
        row["audit_over_solve"] = round(row["audit_ms"]["median"] / row["solve_ms"]["median"], 4)
        row["prune_over_solve"] = round(row["prune_ms"]["median"] / row["solve_ms"]["median"], 4)
        print(json.dumps(row), flush=True)
        s.close()


if __name__ == "__main__":
    main()
