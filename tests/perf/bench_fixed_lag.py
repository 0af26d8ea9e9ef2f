#!/usr/bin/env python3
"""What option "prior_information_structured" buys a fixed-lag caller: translation-only chains of 10 poses with 4 anchors each and the
rank-1 prior that loc_window_marginal_prior_host left on pose 0 after one slide, numeric Jacobians, device-resident batches.

Per batch size, alternating in one process, median of --reps with the spread (min .. max):
  solve_general      the resident solve with the option 0      (window_lm_kernel<.., PINFO>)
  solve_structured   the resident solve with the option 1      (wave3_lm_kernel<1, true>)
  solve_floor        the same batch without any table          (wave3_lm_kernel<1, false>; the priors' diagonals stand in)
  cov_structured     covariance_resident with the option 1     (covariance_kernel<3, 1, false, true>)
  cov_envelope       ... with the option 0 and covariance_general (envelope_covariance_kernel)
  slide_*            one full slide on the host path, wall clock: solve, marginal prior of pose 0, re-pack of the next window (numpy), solve
HIP events around the launches for the solves and the covariances (loc_window_timing_*, loc_window_last_covariance_ms).
Prints one JSON line per batch size.

    python tests/perf/bench_fixed_lag.py [--batches 65536,4096] [--reps 7]
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

W, DISTINCT = 10, 256
OPTION = "prior_information_structured"


def _stats(xs):
    return {"median": round(float(np.median(xs)), 4), "min": round(float(min(xs)), 4), "max": round(float(max(xs)), 4)}


def _after_one_slide(la, F):
    """DISTINCT windows of poses 1 .. 10 with the marginal prior of pose 0 on their first pose, the windows of poses 2 .. 11 after the next
    slide (the structure and measurements the timed re-pack fills), and the ranks of the carried priors"""
    chains = [F.Chain(8800 + i, W + 2, 4) for i in range(DISTINCT)]
    s = la.WindowSolver(F.ANCH, DISTINCT, *F.window_caps(W), jacobian="numeric")
    g = F.first_window(la, chains, W)
    s.solve(g)
    slot, prior, _, _, rank, status = s.marginal_prior(g, 0)
    assert not status.any() and (slot == 1).all()
    base = F.next_window(la, g, chains, 1, W, slot, prior)
    g = base.tile(DISTINCT)
    s.solve(g)
    slot, prior, _, _, _, status = s.marginal_prior(g, 0)
    s.close()
    assert not status.any() and (slot == 1).all()
    return base, F.next_window(la, g, chains, 2, W, slot, prior), rank


def _repack(prev, template, slot, prior):
    """the window after a slide, vectorised: tests/_fixed_lag.next_window's result written into `template`, which already has that window's
    structure, measurements and the new pose's estimate"""
    template.poses[:, :W - 1, 9:] = prev.poses[:, 1:W, 9:]
    template.p_val[:, 0, :12] = prior[:, :12]
    template.p_val[:, 0, 12:] = prior[:, 12:].reshape(-1, 6, 6)[:, np.arange(6), np.arange(6)]
    template.p_info[:, 0] = prior[:, 12:]
    return template


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="65536,4096")
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    import torch
    import localization_amd as la
    import _fixed_lag as F
    base, after, rank = _after_one_slide(la, F)
    for B in (int(x) for x in args.batches.split(",")):
        wb = base.tile(B)
        bare = base.tile(B)
        bare.p_info = None                       # (add_prior_row left diag(W) in p_val: the floor's priors)
        a = la.WindowSolver(F.ANCH, B, *wb.caps, jacobian="numeric")
        f = la.WindowSolver(F.ANCH, B, *wb.caps, jacobian="numeric")
        a.set_option(OPTION, 1)
        a.upload(wb); f.upload(bare)
        a.solve_resident(); f.solve_resident()
        cov = torch.empty((B, W, 36), dtype=torch.float64, device="cuda")
        mask = torch.empty((B, W), dtype=torch.int32, device="cuda")
        status = torch.empty((B,), dtype=torch.int32, device="cuda")
        t = {k: [] for k in ("solve_general", "solve_structured", "solve_floor", "cov_structured", "cov_envelope")}
        kinds = {}

        def solve(s, key):
            s.timing_begin(1)
            s.solve_resident()
            t[key].append(s.timing_end()[1])
            kinds[key] = s.last_kernel_kind()

        def covariance(key):
            a.covariance_resident(cov, mask, status)   # (the first call after a switch classifies the batch again: not timed)
            a.covariance_resident(cov, mask, status)
            t[key].append(a.last_covariance_ms())

        for _ in range(args.reps):
            a.set_option(OPTION, 0); a.set_option("covariance_general", 1)
            solve(a, "solve_general")
            covariance("cov_envelope")
            a.set_option(OPTION, 1); a.set_option("covariance_general", 0)
            solve(a, "solve_structured")
            covariance("cov_structured")
            solve(f, "solve_floor")
        torch.cuda.synchronize()
        assert not (status.cpu() != 0).any()
        f.close()
        # one full slide on the host path, both settings alternating
        slide = {"slide_general": [], "slide_structured": []}
        parts = {}
        template = after.tile(B)
        for _ in range(args.reps):
            for structured, key in ((0, "slide_general"), (1, "slide_structured")):
                a.set_option(OPTION, structured)
                g = base.tile(B)
                t0 = time.perf_counter()
                a.solve(g)
                t1 = time.perf_counter()
                out = a.marginal_prior(g, 0)
                t2 = time.perf_counter()
                nxt = _repack(g, template, out[0], out[1])
                t3 = time.perf_counter()
                a.solve(nxt)
                t4 = time.perf_counter()
                slide[key].append((t4 - t0) * 1e3)
                parts.setdefault(key, []).append([(t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t4 - t3) * 1e3])
                kinds[key] = a.last_kernel_kind()
        a.close()
        row = {"windows": B, "poses": W, "prior_rank_1_share": round(float((rank == 1).mean()), 3), "reps": args.reps, "kernels": kinds}
        row.update({k: _stats(v) for k, v in t.items()})
        row.update({k: _stats(v) for k, v in slide.items()})
        row.update({k + "_parts_median_ms[solve,marginal,repack,solve]": [round(float(x), 3) for x in np.median(np.array(v), axis=0)] for k, v in parts.items()})
        row["structured_over_floor"] = round(row["solve_structured"]["median"] / row["solve_floor"]["median"], 4)
        row["general_over_structured"] = round(row["solve_general"]["median"] / row["solve_structured"]["median"], 2)
        row["envelope_over_chain_pass"] = round(row["cov_envelope"]["median"] / row["cov_structured"]["median"], 2)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
