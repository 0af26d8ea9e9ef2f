#!/usr/bin/env python3
"""Secondary measurements (not the headline bench, nothing is gated on them): what option "upload_dev_structures" buys a caller whose
tables live on the device, at BASELINE config 4's shape (1 024 hypotheses x (256 + 10) poses: arrow3_lm_kernel) and config 5's
(16 384 windows x 64 poses: tree_wave_kernel).  One run, one JSON line per shape:

    python tests/perf/bench_upload_dev_structures.py [--shape selfcal|pose64|both] [--batch B] [--repeats R] [--solves K]

  upload_dev_on_ms / upload_dev_off_ms   the loc_window_upload_dev call, option on / off (host clock, the call is synchronous)
  upload_pinned_ms                       loc_window_upload from page-locked host arrays
  d2h_upload_ms                          the eight tables device -> page-locked host, then loc_window_upload
  bracket_on_ms / bracket_off_ms         loc_window_last_covariance_ms after the call: off = the admit pass's two launches; on = admission,
                                         the device-to-device copy and the structure (+ pack) launches
  d2d_copy_ms                            the eight tables device -> device alone (torch), for reading the bracket
  structure_launches_ms                  bracket_on - bracket_off - d2d_copy: the structure / reduce / pack launches and the host's read-back gap
  solve_on_ms / solve_off_ms             one resident solve, option on (the structured kernel) / off (window_lm_kernel), HIP events
  first_cov_on_ms / first_cov_off_ms     the first loc_window_covariance_resident call after the solve, to completion (host clock): off copies
                                         every table back to classify the batch (LOC_ERR_UNSUPPORTED there is reported as null)
Medians over --repeats calls (the first call of each kind, which allocates, is dropped)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from localization_amd.window import WindowBatch

TABLES = WindowBatch.TABLES


def batch_of(shape, B):
    """the shape's batch: a few windows built edge by edge (bench_window.py), tiled to B with every window's estimates perturbed"""
    import localization_amd as la
    import bench_window as W
    rng = np.random.default_rng(5)
    if shape == "pose64":
        wb, _, anchors, _ = W.build_pose64(B, rng, n_graphs=0)
        return wb, anchors
    small, _, anchors, _ = W.build_selfcal(4, rng)
    wb = small.tile(B)
    wb.poses[:, :, 9:] += rng.normal(0.0, 0.02, wb.poses[:, :, 9:].shape)
    return wb, np.zeros((1, 3))


def median_ms(f, repeats):
    out = []
    for k in range(repeats + 1):
        t = time.perf_counter()
        f()
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out[1:])


def measure(shape, B, repeats, solves):
    import torch
    import localization_amd as la
    wb, anchors = batch_of(shape, B)
    dev = [torch.from_numpy(np.ascontiguousarray(getattr(wb, n))).cuda() for n in TABLES]
    pinned = [torch.from_numpy(np.ascontiguousarray(getattr(wb, n))).pin_memory() for n in TABLES]
    host = la.WindowBatch.__new__(la.WindowBatch)
    host.__dict__.update(wb.__dict__)
    for n, t in zip(TABLES, pinned):
        setattr(host, n, t.numpy())
    torch.cuda.synchronize()
    r = dict(shape=shape, batch=B, caps=list(wb.caps))
    solvers = {}
    for on in (1, 0):
        s = la.WindowSolver(anchors, B, *wb.caps, jacobian="analytic")
        s.set_option("upload_dev_structures", on)
        solvers[on] = s
        tag = "on" if on else "off"
        brackets = []

        def call():
            s.upload_dev(*dev)
            brackets.append(s.last_covariance_ms())
        r[f"upload_dev_{tag}_ms"] = median_ms(call, repeats)
        r[f"bracket_{tag}_ms"] = statistics.median(brackets[1:])
        s.solve_resident(); torch.cuda.synchronize()
        r[f"kernel_{tag}"] = s.last_kernel_kind()
        assert s.L.loc_window_timing_begin(s.h, solves) == 0
        for _ in range(solves):
            s.solve_resident()
        n, total, avg = C.c_int32(), C.c_double(), C.c_double()
        assert s.L.loc_window_timing_end(s.h, C.byref(n), C.byref(total), C.byref(avg)) == 0
        r[f"solve_{tag}_ms"] = avg.value
        cov = torch.zeros((B, wb.caps[0], 36), dtype=torch.float64, device="cuda")
        mask = torch.zeros((B, wb.caps[0]), dtype=torch.int32, device="cuda")
        status = torch.zeros((B,), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        t = time.perf_counter()
        try:
            s.covariance_resident(cov, mask, status)
            torch.cuda.synchronize()
            r[f"first_cov_{tag}_ms"] = (time.perf_counter() - t) * 1e3
        except la.LocalizationAmdError:
            r[f"first_cov_{tag}_ms"] = None
    h = la.WindowSolver(anchors, B, *wb.caps, jacobian="analytic")
    r["upload_pinned_ms"] = median_ms(lambda: h.upload(host), repeats)

    def d2h_upload():
        for t, src in zip(pinned, dev):
            t.copy_(src, non_blocking=True)
        torch.cuda.synchronize()
        h.upload(host)
    r["d2h_upload_ms"] = median_ms(d2h_upload, repeats)
    twins = [torch.empty_like(t) for t in dev]

    def d2d():
        for t, src in zip(twins, dev):
            t.copy_(src, non_blocking=True)
        torch.cuda.synchronize()
    r["d2d_copy_ms"] = median_ms(d2d, repeats)
    r["structure_launches_ms"] = r["bracket_on_ms"] - r["bracket_off_ms"] - r["d2d_copy_ms"]
    for s in list(solvers.values()) + [h]:
        s.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="both", choices=["selfcal", "pose64", "both"])
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--solves", type=int, default=3)
    args = ap.parse_args()
    for shape, B in (("selfcal", 1024), ("pose64", 16384)):
        if args.shape in (shape, "both"):
            print(json.dumps(measure(shape, args.batch or B, args.repeats, args.solves)), flush=True)


if __name__ == "__main__":
    main()
