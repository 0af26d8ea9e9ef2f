#!/usr/bin/env python3
"""Secondary measurements (not the headline bench, nothing is gated on them): option "forest_groups_covariance" at BASELINE config 5's shape,
16 384 windows x 64 poses, resident, with the batch cut into G topologies (tests/perf/bench_forest_groups.py's batches).  One JSON line per
(Jacobian mode, G):

    python tests/perf/bench_forest_groups_covariance.py [--batch B] [--groups 1,8,256,16384] [--jacobian both|numeric|analytic] [--rounds R] [--calls K]

Four arms ALTERNATING for R rounds in one process after a warm-up round, K calls per arm and round, HIP events (loc_window_last_covariance_ms;
the solve: loc_window_timing_*); median over the rounds, and [min, max] as *_spread:
  groups_ms     loc_window_covariance_resident on forest_covariance_kernel<groups> (both options on; the block of the upload)
  envelope_ms   the same resident batch on the envelope pass (option "covariance_general", "forest_groups_covariance" 0)
  control_ms    the one-topology batch (equal anchors) on forest_covariance_kernel
  solve_ms      the mixed batch's resident solve (tree_wave_kernel<groups>)
  joint_ms      the joint call of the first arm with eight leaf - key pairs per window
and on the host clock, call to completion:
  first_call_ms / later_call_ms       the first covariance call after the upload and the median of the later ones, block of the upload
  first_call_own_ms                   the first call on a batch uploaded with "forest_groups" 0 and the options switched on afterwards: the copy-back, the
                                      structure tests, building and sending the groups block"""
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

from bench_forest_groups import ANCH, T, build, parents_of, timed_solves  # noqa: E402

NPAIR = 8


def handle(wb, jac, groups, gcov, general=0):
    import localization_amd as la
    s = la.WindowSolver(ANCH, wb.B, *wb.caps, jacobian=jac, bw_max=T - 1)
    s.set_option("forest_groups", groups)
    s.set_option("forest_groups_covariance", gcov)
    s.set_option("covariance_general", general)
    s.upload(wb)
    s.solve_resident()
    return s


def wall_ms(torch, call):
    torch.cuda.synchronize()
    t = time.perf_counter()
    call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def measure(wb, control, G, jac, rounds, calls):
    import torch
    dev = torch.device("cuda", 0)
    B = wb.B
    out = (torch.zeros((B, T, 36), dtype=torch.float64, device=dev), torch.zeros((B, T), dtype=torch.int32, device=dev), torch.zeros((B,), dtype=torch.int32, device=dev))
    cross = torch.zeros((B, NPAIR, 36), dtype=torch.float64, device=dev)
    par = np.stack([parents_of(g) for g in range(G)])[np.arange(B) % G]
    leaves = T - 1 - np.arange(NPAIR)
    pairs = np.ascontiguousarray(np.stack([np.broadcast_to(leaves, (B, NPAIR)), par[:, leaves]], axis=2).astype(np.int32))
    counts = np.full(B, NPAIR, dtype=np.int32)
    r = {}
    hs = {"groups": handle(wb, jac, 1, 1), "envelope": handle(wb, jac, 1, 0, 1), "control": handle(control, jac, 0, 0)}
    r["n_groups"], r["table_bytes"] = hs["groups"].forest_groups()
    r["first_call_ms"] = wall_ms(torch, lambda: hs["groups"].covariance_resident(*out))
    r["later_call_ms"] = statistics.median(wall_ms(torch, lambda: hs["groups"].covariance_resident(*out)) for _ in range(5))
    times = {k: [] for k in ("groups", "envelope", "control", "solve", "joint")}
    for rnd in range(rounds + 1):                                                        # (round 0 warms every arm up)
        for tag in ("groups", "envelope", "control", "solve", "joint"):
            s = hs["groups" if tag in ("solve", "joint") else tag]
            if tag == "solve":
                ms = timed_solves(s, calls)
            else:
                ms = 0.0
                for _ in range(calls):
                    if tag == "joint":
                        s.joint_covariance_resident(pairs, counts, *out, cross)
                    else:
                        s.covariance_resident(*out)
                    ms += s.last_covariance_ms() / calls
            if rnd:
                times[tag].append(ms)
    for tag, ts in times.items():
        r[f"{tag}_ms"] = statistics.median(ts)
        r[f"{tag}_spread"] = [min(ts), max(ts)]
    r["pass_groups"], r["pass_envelope"], r["pass_control"] = (hs[k].last_covariance_kind() for k in ("groups", "envelope", "control"))
    r["kernel_solve"] = hs["groups"].last_kernel_kind()
    r["singular_windows"] = int((out[2] != 0).sum().item())
    r["envelope_over_groups"] = r["envelope_ms"] / r["groups_ms"]
    r["groups_over_control"] = r["groups_ms"] / r["control_ms"]
    for s in hs.values():
        s.close()
    # the covariance's own block: uploaded ungrouped, the options switched on afterwards
    s = handle(wb, jac, 0, 0)
    s.set_option("forest_groups", 1)
    s.set_option("forest_groups_covariance", 1)
    r["first_call_own_ms"] = wall_ms(torch, lambda: s.covariance_resident(*out))
    r["later_call_own_ms"] = statistics.median(wall_ms(torch, lambda: s.covariance_resident(*out)) for _ in range(5))
    r["pass_own"] = s.last_covariance_kind()
    s.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--groups", default="1,8,256,16384")
    ap.add_argument("--jacobian", default="both", choices=["both", "numeric", "analytic"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2)
    args = ap.parse_args()
    B = args.batch
    modes = ["numeric", "analytic"] if args.jacobian == "both" else [args.jacobian]
    control = build(B, 1, equal_anchors=True)
    for G in (min(int(x), B) for x in args.groups.split(",")):
        wb = build(B, G)
        for jac in modes:
            r = dict(shape="pose64", batch=B, jacobian=jac, G=G)
            r.update(measure(wb, control, G, jac, args.rounds, args.calls))
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
