#!/usr/bin/env python3
"""What the resident slide (loc_window_slide_resident) buys a fixed-lag caller: bench_fixed_lag.py's windows (translation-only chains of 10
poses, 4 anchors each, the rank-1 prior of an earlier slide on pose 0, numeric Jacobians, option "prior_information_structured" on).

Per batch size, the two cycles alternating in one process, median of --reps with the spread (min .. max):
  cycle_resident     solve_resident, slide_resident, solve_resident, stream synchronised          wall clock
  cycle_resident_dl  ... and the solved poses downloaded (what the host cycle hands back anyway)     wall clock
  cycle_host         bench_fixed_lag.py's slide: solve, marginal_prior, numpy re-pack, solve         wall clock (the parent's way: the yardstick)
  slide_launches     the slide's two launches (marginal pass + re-pack kernel)                        HIP events (loc_window_last_covariance_ms)
  marginal_pass      loc_window_marginal_prior_host's launch on the same windows                      HIP events
  solve_kernel       the resident solve's launch                                                      HIP events (loc_window_timing_*)
  slide_host_share   the time loc_window_slide_resident itself takes to return: admission, the mirror pass, staging    wall clock
Every resident cycle starts from a fresh upload of the same batch (not timed), so that each one slides the same windows.
Prints one JSON line per batch size.

    python tests/perf/bench_resident_slide.py [--batches 65536,4096] [--reps 7]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_fixed_lag as H   # noqa: E402  (the host cycle and its windows)

W = H.W


def _new_rows(after, na=4):
    """the rows bench_fixed_lag's `after` windows have on their last pose: the appended pose, its anchor ranges and its link"""
    B, n = after.B, na + 1
    nr = int(after.counts[0, 1])
    assert (after.counts[:, 1] == nr).all()
    r_idx, r_val = after.r_idx[:, nr - n:nr].copy(), after.r_val[:, nr - n:nr].copy()
    assert ((r_idx[:, :, 0] == W - 1) | (r_idx[:, :, 1] == W - 1)).all()
    return after.poses[:, W - 1].copy(), (np.full(B, n, dtype=np.int32), r_idx, r_val)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="65536,4096")
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    import torch
    import localization_amd as la
    import _fixed_lag as F
    base, after, _ = H._after_one_slide(la, F)
    for B in (int(x) for x in args.batches.split(",")):
        wb, template = base.tile(B), after.tile(B)
        pose, ranges = _new_rows(template)
        r = la.WindowSolver(F.ANCH, B, *wb.caps, jacobian="numeric")
        h = la.WindowSolver(F.ANCH, B, *wb.caps, jacobian="numeric")
        for s in (r, h):
            s.set_option(H.OPTION, 1)
        r.set_option("resident_slide", 1)
        out = la.WindowBatch(B, *wb.caps)
        t = {k: [] for k in ("cycle_resident", "cycle_resident_dl", "cycle_host", "slide_launches", "marginal_pass", "solve_kernel", "slide_host_share")}
        kinds = {}
        for rep in range(args.reps + 1):   # (the first round warms both paths up: allocations, the first launches)
            r.upload(wb)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r.timing_begin(2)
            r.solve_resident()
            t1 = time.perf_counter()
            r.slide_resident(pose, ranges)
            t2 = time.perf_counter()
            r.solve_resident()
            solve_ms = r.timing_end()[2]
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            r.download(out)
            t4 = time.perf_counter()
            kinds["resident"] = r.last_kernel_kind()
            g = base.tile(B)
            u0 = time.perf_counter()
            h.solve(g)
            m = h.marginal_prior(g, 0)
            marginal_ms = h.last_covariance_ms()
            nxt = H._repack(g, template, m[0], m[1])
            h.solve(nxt)
            u1 = time.perf_counter()
            kinds["host"] = h.last_kernel_kind()
            if rep == 0:
                continue
            t["cycle_resident"].append((t3 - t0) * 1e3); t["cycle_resident_dl"].append((t4 - t0) * 1e3); t["cycle_host"].append((u1 - u0) * 1e3)
            t["slide_launches"].append(r.last_covariance_ms()); t["marginal_pass"].append(marginal_ms); t["solve_kernel"].append(solve_ms)
            t["slide_host_share"].append((t2 - t1) * 1e3)
        # (both cycles end on the same graph; the host cycle's re-pack stores every kept smoothness edge the other way round, so not on the same bits)
        # (ten LM iterations do not converge every one of these windows, and two stored orders take two damping paths)
        d = np.abs(out.poses[:, :W, 9:] - nxt.poses[:, :W, 9:])
        diff = {"max": float(d.max()), "median": float(np.median(d))}
        r.close(); h.close()
        row = {"windows": B, "poses": W, "reps": args.reps, "kernels": kinds, "largest_pose_difference_between_the_cycles_m": diff}
        row.update({k: H._stats(v) for k, v in t.items()})
        row["host_over_resident"] = round(row["cycle_host"]["median"] / row["cycle_resident"]["median"], 2)
        row["resident_over_kernels_sum"] = round(row["cycle_resident"]["median"] / (2 * row["solve_kernel"]["median"] + row["slide_launches"]["median"]), 2)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
