#!/usr/bin/env python3
"""What the resident plain-drop slide (loc_window_slide_plain_resident_dev) buys a fixed-lag caller of 6-DoF chain windows over the only way the
handle offered before it: loc_window_download_tables, a re-pack in numpy, loc_window_upload.  Windows: cfg/uwb_imu.yaml's (12 poses; an
anchor range with a lever arm, the smoothness edge and an IMU rotation prior per pose; wave6_lm_kernel) and cfg/uwb_twist.yaml's (15 poses;
an anchor range, the smoothness edge and an EdgeSE3 per pair; wave6_lm_kernel<SE3>), numeric Jacobians; 256 distinct windows tiled to the batch.
The two cycles alternate in one process; median of --reps with the spread (min .. max).

Per shape and batch size:
  cycle_resident       solve_resident, slide_plain_resident_dev, solve_resident, stream synchronised                       wall clock
  cycle_host_path      solve_resident, download_tables, the re-pack in numpy (vectorised), upload, solve_resident           wall clock
  download_tables / numpy_repack / upload    of that: the three steps between its two solves (the solved poses' download apart)     wall clock
  slide_launch         the slide kernel alone                                                                               HIP events (loc_window_last_covariance_ms)
  solve_kernel_ms      the solve kernel alone on the slid batch, in the same run                                           HIP events (loc_window_timing_*)
Every cycle starts from a fresh upload of the same batch (not timed); the new rows sit in torch device tensors made once (the host path reads
the same rows from numpy).  The two cycles must end on the same bits (asserted).  Prints one JSON line per shape and batch size.

    python tests/perf/bench_resident_slide_plain.py [--batches 65536,4096] [--reps 7] [--shapes uwb_imu,uwb_twist]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DISTINCT = 256
SHAPES = {"uwb_imu": dict(T=12, se3=0, priors=1), "uwb_twist": dict(T=15, se3=1, priors=0)}
from localization_amd.window import WindowBatch

TABLES = WindowBatch.TABLES


def _stats(xs):
    return {"median": round(float(np.median(xs)), 4), "min": round(float(min(xs)), 4), "max": round(float(max(xs)), 4)}


def _tile(a, B):
    return np.ascontiguousarray(np.concatenate([a] * -(-B // len(a)))[:B])


def _repack_numpy(wb, x, pose, ranges, priors, se3):
    """the plain drop of a batch of FULL, equally built windows, vectorised over the batch (a caller's host path at its best): slot 0's rows go
    by mask, the rest is renumbered, the new rows are appended; poses: the solved estimates x"""
    B = wb.B
    out = type(wb)(B, *wb.caps)
    out.poses[:, :-1] = x[:, 1:]; out.poses[:, -1] = pose
    out.counts[:] = wb.counts
    for idx, val, new, width in ((wb.r_idx, wb.r_val, ranges, 2), (wb.s_idx, wb.s_val, se3, 2), (wb.p_idx[:, :, None], wb.p_val, priors, 1)):
        if idx.shape[1] == 0 or new is None:
            continue
        keep = (idx[:, :, :width] != 0).all(axis=2)
        n_keep = int(keep[0].sum())
        assert (keep.sum(axis=1) == n_keep).all()
        order = np.argsort(~keep, axis=1, kind="stable")[:, :n_keep]
        moved = np.take_along_axis(idx, order[:, :, None], axis=1).copy()
        moved[:, :, :width] -= (moved[:, :, :width] > 0)
        o_idx, o_val = (out.p_idx[:, :, None], out.p_val) if width == 1 else ((out.r_idx, out.r_val) if idx is wb.r_idx else (out.s_idx, out.s_val))
        o_idx[:, :n_keep] = moved
        o_val[:, :n_keep] = np.take_along_axis(val, order[:, :, None], axis=1)
        n_new = new[1].shape[1]
        if width == 1:
            o_idx[:, n_keep:n_keep + n_new, 0] = wb.caps[0] - 1; o_val[:, n_keep:n_keep + n_new] = new[1]
        else:
            o_idx[:, n_keep:n_keep + n_new] = new[1]; o_val[:, n_keep:n_keep + n_new] = new[2]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="65536,4096")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="uwb_imu,uwb_twist")
    args = ap.parse_args()
    import torch
    import localization_amd as la
    import _slide_plain_ref as P
    dev = torch.device("cuda", 0)
    for shape in args.shapes.split(","):
        spec = SHAPES[shape]
        T = spec["T"]
        streams = [P.Stream(8800 + i, T + 1, 1, spec["priors"], spec["se3"]) for i in range(DISTINCT)]
        caps = P.caps_of(T, 1, spec["priors"], spec["se3"])
        base = P.window_batch(la, streams, [T] * DISTINCT, caps)
        pose0, ranges0, priors0, se30 = P.new_rows(streams, [T] * DISTINCT, [T - 1] * DISTINCT)
        for B in (int(x) for x in args.batches.split(",")):
            wb = la.WindowBatch(B, *caps)
            for name in TABLES:
                getattr(wb, name)[:] = _tile(getattr(base, name), B)
            pose = _tile(pose0, B)
            ranges, priors, se3 = (tuple(_tile(a, B) for a in x) for x in (ranges0, priors0, se30))
            assert (ranges[0] == ranges[0][0]).all() and (priors[0] == priors[0][0]).all() and (se3[0] == se3[0][0]).all()   # (equally built windows)
            h_ranges = (ranges[0], ranges[1][:, :int(ranges[0][0])], ranges[2][:, :int(ranges[0][0])])
            h_priors = None if not spec["priors"] else (priors[0], priors[1][:, :int(priors[0][0])])
            h_se3 = None if not spec["se3"] else (se3[0], se3[1][:, :int(se3[0][0])], se3[2][:, :int(se3[0][0])])
            d = la.WindowSolver(P.ANCH, B, *caps, jacobian="numeric")
            h = la.WindowSolver(P.ANCH, B, *caps, jacobian="numeric")
            d.set_option("resident_slide", 1)
            to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            t_pose, t_ranges, t_priors, t_se3 = to(pose), tuple(to(a) for a in ranges), tuple(to(a) for a in priors), tuple(to(a) for a in se3)
            admit = torch.zeros(B, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            out_d, out_h, x = la.WindowBatch(B, *caps), la.WindowBatch(B, *caps), la.WindowBatch(B, *caps)
            t = {k: [] for k in ("cycle_resident", "cycle_host_path", "download_tables", "numpy_repack", "upload", "slide_launch", "solve_kernel_ms")}
            for rep in range(args.reps + 1):   # (the first round warms both paths up: allocations, the first launches)
                d.upload(wb)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                d.solve_resident()
                d.slide_plain_resident_dev(t_pose, t_ranges, t_priors, t_se3, out=(None, admit))
                d.solve_resident()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                d.timing_begin(1)   # (not part of a cycle: the solve kernel alone, on the slid batch)
                d.solve_resident()
                solve_ms = d.timing_end()[1]
                h.upload(wb)
                torch.cuda.synchronize()
                u0 = time.perf_counter()
                h.solve_resident()
                h.download(x)
                ua = time.perf_counter()
                now = h.download_batch()
                u1 = time.perf_counter()
                nxt = _repack_numpy(now, x.poses, pose, h_ranges, h_priors, h_se3)
                u2 = time.perf_counter()
                h.upload(nxt)
                u3 = time.perf_counter()
                h.solve_resident()
                torch.cuda.synchronize()
                u4 = time.perf_counter()
                if rep == 0:
                    assert not admit.cpu().numpy().any()
                    continue
                t["cycle_resident"].append((t1 - t0) * 1e3); t["slide_launch"].append(d.last_covariance_ms()); t["solve_kernel_ms"].append(solve_ms)
                t["cycle_host_path"].append((u4 - u0) * 1e3); t["download_tables"].append((u1 - ua) * 1e3)
                t["numpy_repack"].append((u2 - u1) * 1e3); t["upload"].append((u3 - u2) * 1e3)
            d.download(out_d); h.download(out_h)
            same = out_d.poses.tobytes() == out_h.poses.tobytes() and out_d.result.tobytes() == out_h.result.tobytes()
            assert same, "the two cycles must end on the same bits"
            kind = d.last_kernel_kind()
            d.close(); h.close()
            row = {"shape": shape, "windows": B, "poses": T, "reps": args.reps, "solve_kernel": kind, "cycles_end_on_the_same_bits": same}
            row.update({k: _stats(v) for k, v in t.items()})
            row["host_path_over_resident"] = round(row["cycle_host_path"]["median"] / row["cycle_resident"]["median"], 2)
            row["slide_launch_over_solve_kernel"] = round(row["slide_launch"]["median"] / row["solve_kernel_ms"]["median"], 3)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
