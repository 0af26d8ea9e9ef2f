#!/usr/bin/env python3
"""What taking the slide's inputs from device arrays (loc_window_slide_resident_dev) buys a fixed-lag caller over the host entry point
(loc_window_slide_resident): bench_resident_slide.py's windows and method — translation-only chains of 10 poses, 4 anchors each, the rank-1
prior of an earlier slide on pose 0, numeric Jacobians, option "prior_information_structured" on; the two cycles alternating in one process,
median of --reps with the spread (min .. max).

Per batch size:
  cycle_dev            solve_resident, slide_resident_dev, solve_resident, stream synchronised                  wall clock
  cycle_host_entry     the same cycle through slide_resident (the parent's way: the yardstick)                     wall clock
  dev_call_return      the time loc_window_slide_resident_dev takes to return (handle checks, two launches)         wall clock
  host_call_return     ... loc_window_slide_resident (admission from the mirror, mirror rewrite, staging copy)       wall clock
  dev_launches         the device entry's two launches (marginal pass + admitting re-pack)                          HIP events (loc_window_last_covariance_ms)
  host_launches        the host entry's two launches (marginal pass + re-pack), in the same run                      HIP events
Every cycle starts from a fresh upload of the same batch (not timed), so that each one slides the same windows; the new rows sit in torch
device tensors made once.  The two cycles must end on the same bits (asserted).  Prints one JSON line per batch size.

    python tests/perf/bench_resident_slide_dev.py [--batches 65536,4096] [--reps 7]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_fixed_lag as H         # noqa: E402  (the windows)
import bench_resident_slide as R    # noqa: E402  (the new rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="65536,4096")
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    import torch
    import localization_amd as la
    import _fixed_lag as F
    base, after, _ = H._after_one_slide(la, F)
    dev = torch.device("cuda", 0)
    for B in (int(x) for x in args.batches.split(",")):
        wb, template = base.tile(B), after.tile(B)
        pose, ranges = R._new_rows(template)
        d = la.WindowSolver(F.ANCH, B, *wb.caps, jacobian="numeric")
        h = la.WindowSolver(F.ANCH, B, *wb.caps, jacobian="numeric")
        for s in (d, h):
            s.set_option(H.OPTION, 1)
            s.set_option("resident_slide", 1)
        t_pose = torch.from_numpy(pose).to(dev)
        t_ranges = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in ranges)
        torch.cuda.synchronize()
        out_d, out_h = la.WindowBatch(B, *wb.caps), la.WindowBatch(B, *wb.caps)
        t = {k: [] for k in ("cycle_dev", "cycle_host_entry", "dev_call_return", "host_call_return", "dev_launches", "host_launches")}
        for rep in range(args.reps + 1):   # (the first round warms both paths up: allocations, the first launches)
            d.upload(wb)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            d.solve_resident()
            t1 = time.perf_counter()
            d.slide_resident_dev(t_pose, t_ranges)
            t2 = time.perf_counter()
            d.solve_resident()
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            h.upload(wb)
            torch.cuda.synchronize()
            u0 = time.perf_counter()
            h.solve_resident()
            u1 = time.perf_counter()
            h.slide_resident(pose, ranges)
            u2 = time.perf_counter()
            h.solve_resident()
            torch.cuda.synchronize()
            u3 = time.perf_counter()
            if rep == 0:
                continue
            t["cycle_dev"].append((t3 - t0) * 1e3); t["dev_call_return"].append((t2 - t1) * 1e3); t["dev_launches"].append(d.last_covariance_ms())
            t["cycle_host_entry"].append((u3 - u0) * 1e3); t["host_call_return"].append((u2 - u1) * 1e3); t["host_launches"].append(h.last_covariance_ms())
        d.download(out_d); h.download(out_h)
        same = out_d.poses.tobytes() == out_h.poses.tobytes() and out_d.result[:, :6].tobytes() == out_h.result[:, :6].tobytes()
        assert same, "the two cycles must end on the same bits"
        kind = d.last_kernel_kind()
        d.close(); h.close()
        row = {"windows": B, "poses": H.W, "reps": args.reps, "solve_kernel": kind, "cycles_end_on_the_same_bits": same}
        row.update({k: H._stats(v) for k, v in t.items()})
        row["host_entry_over_dev"] = round(row["cycle_host_entry"]["median"] / row["cycle_dev"]["median"], 2)
        row["dev_launches_over_host_launches"] = round(row["dev_launches"]["median"] / row["host_launches"]["median"], 3)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
