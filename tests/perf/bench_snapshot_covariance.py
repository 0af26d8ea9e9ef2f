#!/usr/bin/env python3
"""Cost of the per-update covariances in the snapshot and fusion solve kernels: the COV = true kernels (loc_snapshot_solve_device_cov,
loc_fusion_solve_device_cov) against the plain ones on the same device-resident inputs.  Cases: cfg2 (65 536 tags x 8 anchors, M_PAD 8,
one lane per tag — the bench.py headline), 16 anchors with two lanes per tag, and cfg3 (fusion: 8 anchors, lever arm, IMU prior); each in
numeric and analytic mode.  Kernel time from HIP events around each launch (loc_*_timing_*), best of --reps, off / on alternating, the
state reset before every launch so that each one solves the same problem.  Prints one JSON line per case.

    python tests/perf/bench_snapshot_covariance.py [--batch 65536] [--epochs 128] [--fusion-epochs 64] [--reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ANCH16 = np.array([[3.0, -3.0, 0.0], [3.0, 3.0, 2.0], [-3.0, 3.0, 0.0], [-3.0, -3.0, 2.0],
                   [3.0, -3.0, 2.0], [3.0, 3.0, 0.0], [-3.0, 3.0, 2.0], [-3.0, -3.0, 0.0],
                   [0.0, -3.0, 1.0], [3.0, 0.0, 1.5], [0.0, 3.0, 0.5], [-3.0, 0.0, 1.2],
                   [1.5, -3.0, 2.0], [3.0, 1.5, 0.2], [-1.5, 3.0, 1.8], [-3.0, -1.5, 0.7]])


def _best(solver, reset, launch_off, launch_on, reps):
    off, on = [], []
    for _ in range(reps):
        for launch, acc in ((launch_off, off), (launch_on, on)):
            reset()
            solver.timing_begin(1)
            launch()
            _, tot, _ = solver.timing_end()
            acc.append(tot)
    return min(off), min(on)


def snapshot_case(la, name, anchors, lpi, jac, B, K, reps):
    import torch
    from localization_amd.synthetic import make_snapshot_stream_torch
    dev = torch.device("cuda", 0)
    s = make_snapshot_stream_torch(B, K, seed=1, device=dev, anchors=anchors)
    sv = la.SnapshotSolver(anchors, B, maximum_iteration=10, distance_outlier=1.0, jacobian=jac, lanes_per_instance=lpi)
    outs = sv.alloc_outputs(K, covariance=True)
    d, e = s["dist_tiles"], s["err_tiles"]
    reset = lambda: sv.set_positions(s["init"])   # noqa: E731
    reset(); sv.solve_device(d, e, *outs[:3]); sv.solve_device(d, e, *outs)   # warm-up of both kernels
    torch.cuda.synchronize()
    off, on = _best(sv, reset, lambda: sv.solve_device(d, e, *outs[:3]), lambda: sv.solve_device(d, e, *outs), reps)
    singular = int((outs[5] != 0).sum())
    sv.close()
    return {"case": name, "jacobian": jac, "tags": B, "epochs": K, "lanes_per_tag": lpi, "anchors": len(anchors),
            "cov_off_ms": round(off, 4), "cov_on_ms": round(on, 4), "on_over_off": round(on / off, 4),
            "updates_per_s_on": round(B * K / on * 1e3), "singular_updates": singular}


def fusion_case(la, jac, B, K, reps):
    import torch
    from localization_amd.snapshot import pack_ranges
    from localization_amd.synthetic import make_fusion_stream
    dev = torch.device("cuda", 0)
    s = make_fusion_stream(B, K, seed=1)
    f = la.FusionSolver(s["anchors"], B, antenna_offset=s["offset"], maximum_iteration=10, distance_outlier=3.0, jacobian=jac)
    d = torch.from_numpy(pack_ranges(s["dist"])).to(dev); e = torch.from_numpy(pack_ranges(s["err"])).to(dev)
    imu = torch.from_numpy(s["imu"]).to(dev)
    outs = f.alloc_outputs(K, covariance=True)
    reset = lambda: f.set_poses(s["init"])   # noqa: E731
    reset(); f.solve_device(d, e, imu, *outs[:3]); f.solve_device(d, e, imu, *outs)
    torch.cuda.synchronize()
    off, on = _best(f, reset, lambda: f.solve_device(d, e, imu, *outs[:3]), lambda: f.solve_device(d, e, imu, *outs), reps)
    singular = int((outs[5] != 0).sum())
    f.close()
    return {"case": "cfg3_fusion_8_anchors_lever_imu", "jacobian": jac, "tags": B, "epochs": K,
            "cov_off_ms": round(off, 4), "cov_on_ms": round(on, 4), "on_over_off": round(on / off, 4),
            "updates_per_s_on": round(B * K / on * 1e3), "singular_updates": singular}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--epochs", type=int, default=128)
    ap.add_argument("--fusion-epochs", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import localization_amd as la
    for jac in ("numeric", "analytic"):
        print(json.dumps(snapshot_case(la, "cfg2_8_anchors_lpi1", ANCH16[:8], 1, jac, args.batch, args.epochs, args.reps)), flush=True)
        print(json.dumps(snapshot_case(la, "16_anchors_lpi2", ANCH16, 2, jac, args.batch, args.epochs, args.reps)), flush=True)
        print(json.dumps(fusion_case(la, jac, args.batch, args.fusion_epochs, args.reps)), flush=True)


if __name__ == "__main__":
    main()
