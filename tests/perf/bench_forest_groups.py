#!/usr/bin/env python3
"""Secondary measurements (not the headline bench, nothing is gated on them): option "forest_groups" at BASELINE config 5's shape, 16 384
windows x 64 poses (one anchor range per pose, one EdgeSE3 to the pose's key), with the batch cut into G topologies.  One JSON line per
(Jacobian mode, G), then one for the uniform control:

    python tests/perf/bench_forest_groups.py [--batch B] [--groups 1,8,256,16384] [--jacobian both|numeric|analytic] [--rounds R] [--solves K]

Topologies: key cadence (a new key every 3 .. 18 poses) and phase (the length of the first key run), 168 combinations; beyond those, bit j of
the topology number re-hangs pose 63 - j on pose 0.  G = 1: one topology, the windows differ in the anchors they range alone.
  twin_ms / general_ms        one resident solve of the SAME batch: option on (tree_wave_kernel<groups>) / off (window_lm_kernel); HIP events
                              (loc_window_timing_*) around K solves, the arms ALTERNATING for R rounds in one process after a warm-up round;
                              median, and [min, max] over the rounds as *_spread
  ratio                       general_ms / twin_ms (medians)
  upload_on_ms / upload_off_ms   loc_window_upload of that batch, option on (grouping + G schedules + their copy) / off (host clock, medians)
  n_groups, table_bytes       loc_window_forest_groups after the upload
control: the one-topology batch (equal anchors) on tree_wave_kernel with the option on and off — the same path, so the two agree within the
spread — and its upload, the figure the mixed uploads are read against."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
from scipy.spatial.transform import Rotation

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

ANCH = np.array([[3, -3, 0.58], [3, 3, 1.97], [-3, 3, 0.54], [-3, -3, 1.76]], dtype=float)
T = 64
COMBOS = [(every, first) for every in range(3, 19) for first in range(1, every + 1)]


def parents_of(topology):
    """parent slot of every pose of topology number `topology` (always a lower slot: a tree)"""
    every, first = COMBOS[topology % len(COMBOS)]
    k = np.arange(T)
    parent = np.where(k < first, 0, ((k - first) // every) * every + first - 1)
    extra = topology // len(COMBOS)
    for j in range(14):
        if extra >> j & 1:
            parent[T - 1 - j] = 0
    parent[0] = -1
    return parent


def build(B, G, seed=5, equal_anchors=False):
    """B windows, window b of topology b % G, every table filled with numpy (no per-edge Python call)"""
    import localization_amd as la
    rng = np.random.default_rng(seed)
    wb = la.WindowBatch(B, T, T, 0, T - 1)
    par = np.stack([parents_of(g) for g in range(G)])[np.arange(B) % G]                  # [B][T]
    tt = np.cumsum(rng.normal(0, 0.05, (B, T, 3)), axis=1) + np.concatenate([rng.uniform(-1.5, 1.5, (B, 1, 2)), np.full((B, 1, 1), 1.1)], axis=2)
    rv = np.cumsum(rng.normal(0, 0.03, (B, T, 3)), axis=1) + rng.normal(0, 0.3, (B, 1, 3))
    tR = Rotation.from_rotvec(rv.reshape(-1, 3)).as_matrix().reshape(B, T, 3, 3)
    eR = (Rotation.from_rotvec(rv.reshape(-1, 3)) * Rotation.from_rotvec(rng.normal(0, 0.02, (B * T, 3)))).as_matrix().reshape(B, T, 9)
    wb.counts[:] = (T, T, 0, T - 1)
    wb.poses[:, :, :9] = eR
    wb.poses[:, :, 9:] = tt + rng.normal(0, 0.05, (B, T, 3))
    k = np.arange(T)
    shift = np.zeros(B, int) if equal_anchors else (np.arange(B) // G) % 4
    a = (k[None, :] + shift[:, None]) % 4
    wb.r_idx[:, :, 0] = k
    wb.r_idx[:, :, 1] = -1 - a
    wb.r_val[:, :, 0] = np.float32(np.linalg.norm(tt - ANCH[a], axis=2) + rng.normal(0, 0.03, (B, T)))
    wb.r_val[:, :, 1] = 1 / 0.055 ** 2
    p = par[:, 1:]                                                                       # edge e joins parent p[e] (vi) and pose e + 1 (vj)
    Rp = np.take_along_axis(tR, p[:, :, None, None], axis=1)
    tp = np.take_along_axis(tt, p[:, :, None], axis=1)
    Zt = np.einsum("beji,bej->bei", Rp, tt[:, 1:] - tp) + rng.normal(0, 0.01, (B, T - 1, 3))
    ZR = np.einsum("beji,bejk->beik", Rp, tR[:, 1:])
    wb.s_idx[:, :, 0] = p
    wb.s_idx[:, :, 1] = k[1:]
    wb.s_idx[:, :, 2] = 1
    wb.s_val[:, :, :9] = ZR.transpose(0, 1, 3, 2).reshape(B, T - 1, 9)                   # Z^-1 as R, t
    wb.s_val[:, :, 9:12] = -np.einsum("beji,bej->bei", ZR, Zt)
    A = rng.normal(size=(B, T - 1, 6, 6))
    info = A @ A.transpose(0, 1, 3, 2) + 6 * np.eye(6)
    info *= (6e4 / np.trace(info, axis1=2, axis2=3))[:, :, None, None]
    wb.s_val[:, :, 12:] = info.reshape(B, T - 1, 36)
    return wb


def timed_solves(s, solves):
    assert s.L.loc_window_timing_begin(s.h, solves) == 0
    for _ in range(solves):
        s.solve_resident()
    n, total, avg = C.c_int32(), C.c_double(), C.c_double()
    assert s.L.loc_window_timing_end(s.h, C.byref(n), C.byref(total), C.byref(avg)) == 0
    return avg.value


def upload_ms(s, wb, repeats=3):
    out = []
    for _ in range(repeats + 1):
        t = time.perf_counter()
        s.upload(wb)
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out[1:])                                                    # (the first upload allocates)


def arms(wb, jac, rounds, solves, kinds):
    """the batch resident on two handles, option on and off; alternating rounds of K timed solves each"""
    import localization_amd as la
    r, hs = {}, {}
    for tag, on in (("on", 1), ("off", 0)):
        s = la.WindowSolver(ANCH, wb.B, *wb.caps, jacobian=jac, bw_max=T - 1)
        s.set_option("forest_groups", on)
        r[f"upload_{tag}_ms"] = upload_ms(s, wb)
        if on:
            r["n_groups"], r["table_bytes"] = s.forest_groups()
        hs[tag] = s
    times = {"on": [], "off": []}
    for rnd in range(rounds + 1):                                                        # (round 0 warms both arms up)
        for tag in ("on", "off"):
            ms = timed_solves(hs[tag], solves)
            if rnd:
                times[tag].append(ms)
    for tag, name in (("on", kinds[0]), ("off", kinds[1])):
        r[f"kernel_{tag}"] = hs[tag].last_kernel_kind()
        r[f"{name}_ms"] = statistics.median(times[tag])
        r[f"{name}_spread"] = [min(times[tag]), max(times[tag])]
        hs[tag].close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--groups", default="1,8,256,16384")
    ap.add_argument("--jacobian", default="both", choices=["both", "numeric", "analytic"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--solves", type=int, default=3)
    args = ap.parse_args()
    B = args.batch
    modes = ["numeric", "analytic"] if args.jacobian == "both" else [args.jacobian]
    batches = {G: build(B, min(G, B)) for G in (int(x) for x in args.groups.split(","))}
    control = build(B, 1, equal_anchors=True)
    for jac in modes:
        for G, wb in batches.items():
            r = dict(shape="pose64", batch=B, jacobian=jac, G=min(G, B))
            r.update(arms(wb, jac, args.rounds, args.solves, ("twin", "general")))
            r["ratio"] = r["general_ms"] / r["twin_ms"]
            print(json.dumps(r), flush=True)
        r = dict(shape="pose64", batch=B, jacobian=jac, G=0, control="one topology, equal anchors: tree_wave_kernel on both arms")
        r.update(arms(control, jac, args.rounds, args.solves, ("uniform_on", "uniform_off")))
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
