#!/usr/bin/env python3
"""What loc_window_upload_dev costs against loc_window_upload ("Upload from device arrays").  Windows: cfg/uwb_only.yaml's (10
poses, translation-only: an anchor range, the smoothness edge and a prior per pose; verdict CHAIN3) and cfg/uwb_twist.yaml's (15 poses; an anchor
range, the smoothness edge and an EdgeSE3 per pair; verdict WAVE6S); 256 distinct windows tiled to the batch.

Per shape and batch size, alternated --rounds times in one process (each round: --reps calls of each, after one warm-up round that is not
counted); median with the spread (min .. max), wall clock around calls that return synchronously:
  upload_dev            upload_dev from torch device tensors
  upload_pinned         loc_window_upload of the same batch from page-locked host arrays                    (a): upload_dev against this
  d2h_then_upload       the eight tables device -> page-locked host, then loc_window_upload                 (b): a caller whose tables are on the device
  d2h                   of that: the copies alone
  h2d                   the bare host-to-device copies of the same bytes; host_passes_ms = upload_pinned - h2d: what loc_window_upload spends
                        on its host passes (validation, structure scans, the mirror)
  admit_launch          the admit pass's two launches alone, HIP events (loc_window_last_covariance_ms)       (c)
  admit_gbs             the bytes the pass must read (counts, the used index rows once, and for a translation-only candidate the lever
                        arms, the poses' rotations and the priors' rotations and rotation information) over admit_launch
Both handles must solve to the same bits afterwards (asserted).  Prints one JSON line per shape and batch size.

    python tests/perf/bench_upload_dev.py [--batches 65536,4096] [--rounds 3] [--reps 5] [--shapes uwb_only,uwb_twist]
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
SHAPES = {"uwb_only": dict(T=10, se3=0, priors=1, chain3=True), "uwb_twist": dict(T=15, se3=1, priors=0, chain3=False)}
from localization_amd.window import WindowBatch

TABLES = WindowBatch.TABLES


def _stats(xs):
    return {"median": round(float(np.median(xs)), 4), "min": round(float(min(xs)), 4), "max": round(float(max(xs)), 4)}


def _tile(a, B):
    return np.ascontiguousarray(np.concatenate([a] * -(-B // len(a)))[:B])


def needed_bytes(wb, chain3):
    """what the admit pass must read of a batch: the counts, every used index row once; for a translation-only candidate also three of a range
    row's five doubles, nine of a pose's twelve and twelve of a prior's eighteen"""
    nv, nr, npr, ns = (wb.counts[:, k].astype(np.int64).sum() for k in range(4))
    total = wb.B * 16 + nr * 8 + npr * 4 + ns * 16
    if chain3:
        total += nr * 24 + nv * 72 + npr * 96
    return int(total)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="65536,4096")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="uwb_only,uwb_twist")
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
        if spec["chain3"]:   # nothing that turns a pose: identity rotations, no lever arm, translation information only
            base.poses[:, :, :9] = np.eye(3).reshape(9)
            base.r_val[:, :, 2:] = 0.0
            base.p_val[:, :, :9] = np.eye(3).reshape(9); base.p_val[:, :, 15:] = 0.0; base.p_val[:, :, 12:15] = 4.0
        for B in (int(x) for x in args.batches.split(",")):
            wb = la.WindowBatch(B, *caps)
            pinned = {}
            for name in TABLES:   # the batch in page-locked host memory (what loc_window_upload reads), and on the device
                pinned[name] = torch.from_numpy(_tile(getattr(base, name), B)).pin_memory()
                setattr(wb, name, pinned[name].numpy())
            d_tab = [pinned[name].to(dev) for name in TABLES]
            back = la.WindowBatch(B, *caps)   # (b)'s destination: page-locked as well
            back_pinned = {name: torch.empty_like(pinned[name]).pin_memory() for name in TABLES}
            for name in TABLES:
                setattr(back, name, back_pinned[name].numpy())
            scratch = [torch.empty_like(t) for t in d_tab]
            a = la.WindowSolver(P.ANCH, B, *caps, jacobian="numeric")
            h = la.WindowSolver(P.ANCH, B, *caps, jacobian="numeric")
            torch.cuda.synchronize()
            t = {k: [] for k in ("upload_dev", "upload_pinned", "d2h_then_upload", "d2h", "h2d", "admit_launch")}
            for rnd in range(args.rounds + 1):   # (round 0 warms every path up: allocations, the first launches)
                for rep in range(args.reps):
                    t0 = time.perf_counter()
                    a.upload_dev(*d_tab)
                    t1 = time.perf_counter()
                    admit_ms = a.last_covariance_ms()
                    t2 = time.perf_counter()
                    h.upload(wb)
                    t3 = time.perf_counter()
                    for name, src in zip(TABLES, d_tab):
                        back_pinned[name].copy_(src, non_blocking=True)
                    torch.cuda.synchronize()
                    t4 = time.perf_counter()
                    h.upload(back)
                    t5 = time.perf_counter()
                    for name, dst in zip(TABLES, scratch):
                        dst.copy_(pinned[name], non_blocking=True)
                    torch.cuda.synchronize()
                    t6 = time.perf_counter()
                    if rnd == 0:
                        continue
                    t["upload_dev"].append((t1 - t0) * 1e3); t["admit_launch"].append(admit_ms); t["upload_pinned"].append((t3 - t2) * 1e3)
                    t["d2h"].append((t4 - t3) * 1e3); t["d2h_then_upload"].append((t5 - t3) * 1e3); t["h2d"].append((t6 - t5) * 1e3)
            for name in TABLES:
                assert back_pinned[name].numpy().tobytes() == pinned[name].numpy().tobytes(), name
            a.solve_resident(); h.solve_resident()
            out_a, out_h = la.WindowBatch(B, *caps), la.WindowBatch(B, *caps)
            a.download(out_a); h.download(out_h)
            same = out_a.poses.tobytes() == out_h.poses.tobytes() and out_a.result.tobytes() == out_h.result.tobytes() and a.last_kernel_kind() == h.last_kernel_kind()
            assert same, "the two uploads must solve to the same bits on the same kernel"
            kind = a.last_kernel_kind()
            a.close(); h.close()
            nbytes = needed_bytes(wb, spec["chain3"])
            row = {"shape": shape, "windows": B, "poses": T, "rounds": args.rounds, "reps": args.reps, "solve_kernel": kind, "same_bits": same,
                   "table_bytes": int(sum(pinned[name].numel() * pinned[name].element_size() for name in TABLES)), "admit_needed_bytes": nbytes}
            row.update({k: _stats(v) for k, v in t.items()})
            row["host_passes_ms"] = round(row["upload_pinned"]["median"] - row["h2d"]["median"], 4)
            row["upload_pinned_over_upload_dev"] = round(row["upload_pinned"]["median"] / row["upload_dev"]["median"], 2)
            row["d2h_then_upload_over_upload_dev"] = round(row["d2h_then_upload"]["median"] / row["upload_dev"]["median"], 2)
            row["admit_gbs"] = round(nbytes / (row["admit_launch"]["median"] * 1e-3) / 1e9, 1)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
