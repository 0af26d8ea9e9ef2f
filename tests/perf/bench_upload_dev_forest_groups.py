#!/usr/bin/env python3
"""Secondary measurements (not the headline bench, nothing is gated on them): what option "upload_dev_forest_groups" buys a caller whose
mixed forest batch lives on the device, at BASELINE config 5's shape (16 384 windows x 64 poses, numeric Jacobians) cut into G topologies
(tests/perf/bench_forest_groups.py builds the batches).  One run, one JSON line per G:

    python tests/perf/bench_upload_dev_forest_groups.py [--batch B] [--groups 1,8,256,16384] [--repeats R] [--rounds N] [--solves K]

  upload_dev_on_ms / upload_dev_off_ms   the loc_window_upload_dev call with "upload_dev_structures" and "forest_groups" 1 and the new option
                                         on / off (host clock, the call is synchronous); off is what the batch took before the option existed
  upload_pinned_ms                       (i) loc_window_upload from page-locked host arrays, "forest_groups" 1
  d2h_upload_ms                          (ii) the eight tables device -> page-locked host, then (i)
  bracket_on_ms / bracket_off_ms         loc_window_last_covariance_ms after the call: admission, the device-to-device copy and the structure
                                         launches; on: the grouping launches as well (and the host's read-back gaps between them)
  groups_launches_ms                     bracket_on - bracket_off: the grouping pass's launches alone
  solve_on_ms / solve_off_ms / solve_host_ms   one resident solve after upload_dev on (tree_wave_kernel<groups>) / off (window_lm_kernel) / after
                                         upload() (tree_wave_kernel<groups>: the same instruction stream as on); HIP events around K solves, the
                                         arms alternating for N rounds after a warm-up round, medians
  first_cov_on_ms / first_cov_off_ms / first_cov_host_ms   the first loc_window_covariance_resident call ("forest_groups_covariance" 1) after a
                                         fresh upload + solve, to completion (host clock): on and host walk the uploaded block, off copies the
                                         tables back and builds a block of its own
  n_groups, table_bytes                  loc_window_forest_groups after upload_dev on (equal to upload()'s: asserted)
Medians over --repeats calls (the first call of each kind, which allocates, is dropped); the first covariance calls are single calls."""
import argparse
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

import bench_forest_groups as FG
from localization_amd.window import WindowBatch

TABLES = WindowBatch.TABLES


def median_ms(f, repeats):
    out = []
    for _ in range(repeats + 1):
        t = time.perf_counter()
        f()
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out[1:])


def measure(B, G, repeats, rounds, solves):
    import torch
    import localization_amd as la
    wb = FG.build(B, G)
    dev = [torch.from_numpy(np.ascontiguousarray(getattr(wb, n))).cuda() for n in TABLES]
    pinned = [torch.from_numpy(np.ascontiguousarray(getattr(wb, n))).pin_memory() for n in TABLES]
    host = la.WindowBatch.__new__(la.WindowBatch)
    host.__dict__.update(wb.__dict__)
    for n, t in zip(TABLES, pinned):
        setattr(host, n, t.numpy())
    torch.cuda.synchronize()
    r = dict(shape="pose64", batch=B, jacobian="numeric", G=G, caps=list(wb.caps))

    def handle(**options):
        s = la.WindowSolver(FG.ANCH, B, *wb.caps, jacobian="numeric", bw_max=FG.T - 1)
        for k, v in dict(forest_groups=1, forest_groups_covariance=1, **options).items():
            s.set_option(k, v)
        return s
    hs = {"on": handle(upload_dev_structures=1, upload_dev_forest_groups=1), "off": handle(upload_dev_structures=1, upload_dev_forest_groups=0), "host": handle()}
    uploads = {"on": lambda: hs["on"].upload_dev(*dev), "off": lambda: hs["off"].upload_dev(*dev), "host": lambda: hs["host"].upload(host)}
    for tag in ("on", "off"):
        brackets = []

        def call():
            uploads[tag]()
            brackets.append(hs[tag].last_covariance_ms())
        r[f"upload_dev_{tag}_ms"] = median_ms(call, repeats)
        r[f"bracket_{tag}_ms"] = statistics.median(brackets[1:])
    r["groups_launches_ms"] = r["bracket_on_ms"] - r["bracket_off_ms"]
    r["upload_pinned_ms"] = median_ms(uploads["host"], repeats)

    def d2h_upload():
        for t, src in zip(pinned, dev):
            t.copy_(src, non_blocking=True)
        torch.cuda.synchronize()
        hs["host"].upload(host)
    r["d2h_upload_ms"] = median_ms(d2h_upload, repeats)
    r["n_groups"], r["table_bytes"] = hs["on"].forest_groups()
    assert hs["on"].forest_groups() == hs["host"].forest_groups(), (hs["on"].forest_groups(), hs["host"].forest_groups())
    times = {tag: [] for tag in hs}
    for rnd in range(rounds + 1):                                                        # (round 0 warms the arms up)
        for tag, s in hs.items():
            ms = FG.timed_solves(s, solves)
            if rnd:
                times[tag].append(ms)
    for tag, s in hs.items():
        r[f"kernel_{tag}"] = s.last_kernel_kind()
        r[f"solve_{tag}_ms"] = statistics.median(times[tag])
        r[f"solve_{tag}_spread"] = [min(times[tag]), max(times[tag])]
    cov = torch.zeros((B, wb.caps[0], 36), dtype=torch.float64, device="cuda")
    mask = torch.zeros((B, wb.caps[0]), dtype=torch.int32, device="cuda")
    status = torch.zeros((B,), dtype=torch.int32, device="cuda")
    for tag, s in hs.items():
        uploads[tag]()                                                                   # a fresh upload: the covariance verdict is open again
        s.solve_resident()
        torch.cuda.synchronize()
        t = time.perf_counter()
        try:
            s.covariance_resident(cov, mask, status)
            torch.cuda.synchronize()
            r[f"first_cov_{tag}_ms"] = (time.perf_counter() - t) * 1e3
            r[f"cov_kind_{tag}"] = s.last_covariance_kind()
        except la.LocalizationAmdError:
            r[f"first_cov_{tag}_ms"] = None
    for s in hs.values():
        s.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--groups", default="1,8,256,16384")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--solves", type=int, default=3)
    args = ap.parse_args()
    for G in (int(x) for x in args.groups.split(",")):
        print(json.dumps(measure(args.batch, min(G, args.batch), args.repeats, args.rounds, args.solves)), flush=True)


if __name__ == "__main__":
    main()
