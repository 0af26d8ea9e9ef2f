#!/usr/bin/env python3
"""Time of a joint covariance call (loc_window_joint_covariance_resident: the marginals and the cross blocks of requested pose pairs) next
to the plain call (loc_window_covariance_resident) on the same device-resident batch in the same run, numeric Jacobians, one row per pass
at the project's shapes:
  chain     65 536 translation-only windows x T = 10, the T - 1 adjacent pairs               (covariance_kernel<3>)
  forest    16 384 key-frame windows x 64 poses (a key every 8), every leaf - key pair      (forest_covariance_kernel)
  arrow     1 024 hypotheses x (256 tag poses + 10 unknown anchors), the 45 anchor pairs     (arrow_covariance_kernel)
  envelope  64 key-frame windows x 500 poses (a key every 10), the pair (newest, T / 2)      (envelope_covariance_kernel)
Both timed with HIP events around the launch (loc_window_last_covariance_ms), alternated, best of --reps; `spread` is the largest relative
distance of a plain rep from the best one.  Prints one JSON line per pass.

    python tests/perf/bench_joint_covariance.py [--reps 7] [--only chain,forest,arrow,envelope] [--plain-only] [--root DIR]

--plain-only times the plain call alone and touches no joint entry point; with --root DIR it loads the package and the library of another
checkout (the parent commit's, built there), so that the plain calls of two builds can be alternated in one run.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _tables(B, per_window):
    npm = max(len(p) for p in per_window)
    pairs = np.zeros((B, npm, 2), dtype=np.int32)
    counts = np.zeros(B, dtype=np.int32)
    for w in range(B):
        p = per_window[w % len(per_window)]
        counts[w] = len(p)
        pairs[w, :len(p)] = p
    return pairs, counts


def _shapes(la):
    """name -> (kernel, shape, batch builder, anchors, solver keywords, options, pairs per distinct window)"""
    from test_gpu_covariance import _observable_batch
    from test_gpu_tree_parity import ANCH as FANCH, _forest_batch
    from test_gpu_window_parity import ANCH
    import _general_cov_inputs as G
    import bench_window as bw

    def chain():
        small = _observable_batch(la, np.random.default_rng(0), 1024, 10, False, False, translation_only=True)
        return small.tile(65536), ANCH, {}, {}, [[(k, k + 1) for k in range(int(nv) - 1)] for nv in small.counts[:, 0]]

    def forest():
        T, every = 64, 8
        small = _forest_batch(la, np.random.default_rng(0), 256, T, every, False)
        key = np.where(np.arange(T) < every, 0, (np.arange(T) // every) * every - 1)
        leaves = [k for k in range(1, T) if k not in set(key.tolist())]
        return small.tile(16384), FANCH, {"bw_max": T - 1}, {}, [[(k, int(key[k])) for k in leaves]]

    def arrow():
        small, _, anchors, nv = bw.build_selfcal(32, np.random.default_rng(21))
        pairs = [[(a, b) for a in range(int(n) - 10, int(n)) for b in range(a + 1, int(n))] for n in small.counts[:, 0]]
        return small.tile(1024), anchors, {"maximum_iteration": 10, "bw_max": nv - 1}, {}, pairs

    def envelope():
        small = G.keyframe_batch(la, 2, 8, 500, 10)
        return small.tile(64), G.ANCH, {}, {"covariance_general": 1}, [[(499, 250)]]

    return {"chain": ("covariance_kernel<3>", "65 536 x T = 10, adjacent pairs", chain),
            "forest": ("forest_covariance_kernel", "16 384 x 64 poses, leaf - key pairs", forest),
            "arrow": ("arrow_covariance_kernel", "1 024 x (256 + 10), anchor - anchor pairs", arrow),
            "envelope": ("envelope_covariance_kernel", "64 x 500 key-frame poses, (newest, T / 2)", envelope)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", default="chain,forest,arrow,envelope")
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--root", default=ROOT)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    for d in ("tests", os.path.join("tests", "perf")):
        sys.path.append(os.path.join(ROOT, d))
    import torch
    import localization_amd as la
    shapes = _shapes(la)
    for name in args.only.split(","):
        kernel, shape, build = shapes[name]
        wb, anchors, kw, opt, per_window = build()
        B, T = wb.B, wb.caps[0]
        s = la.WindowSolver(anchors, B, *wb.caps, jacobian="numeric", **kw)
        for k, v in opt.items():
            s.set_option(k, v)
        s.upload(wb)
        s.solve_resident()
        pairs, counts = _tables(B, per_window)
        npm = pairs.shape[1]
        cov = torch.empty((B, T, 36), dtype=torch.float64, device="cuda")
        mask = torch.empty((B, T), dtype=torch.int32, device="cuda")
        status = torch.empty((B,), dtype=torch.int32, device="cuda")
        cross = torch.empty((B, npm, 36), dtype=torch.float64, device="cuda")
        s.covariance_resident(cov, mask, status)                                     # (the first calls classify and allocate)
        if not args.plain_only:
            s.joint_covariance_resident(pairs, counts, cov, mask, status, cross)
        plain_ms, joint_ms = [], []
        for _ in range(args.reps):
            s.covariance_resident(cov, mask, status)
            plain_ms.append(s.last_covariance_ms())
            if not args.plain_only:
                s.joint_covariance_resident(pairs, counts, cov, mask, status, cross)
                joint_ms.append(s.last_covariance_ms())
        torch.cuda.synchronize()
        row = {"pass": kernel, "shape": shape, "windows": B, "library": la.library_path() if args.root != ROOT else "this checkout",
               "plain_ms": round(min(plain_ms), 4), "plain_spread": round(max(plain_ms) / min(plain_ms) - 1, 4),
               "singular_windows": int((status.cpu() != 0).sum())}
        if not args.plain_only:
            row.update({"pairs_per_window": int(counts.max()), "joint_ms": round(min(joint_ms), 4), "joint_over_plain": round(min(joint_ms) / min(plain_ms), 3)})
        print(json.dumps(row), flush=True)
        s.close()


if __name__ == "__main__":
    main()
