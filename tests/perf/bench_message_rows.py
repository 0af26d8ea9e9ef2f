#!/usr/bin/env python3
"""What building a resident batch's next pose and factors ON THE DEVICE (loc_window_push_messages_resident_dev: window_message_kernel.hip, then
the resident slide) buys over the way every caller built them before: download the solved poses, build the rows in numpy from the same raw
messages, copy them to the device, call the existing slide_*_resident_dev.  Windows at their lag: cfg/uwb_only.yaml's (10 poses, translation
only, chain3 verdict, the marginal carry, option "prior_information_structured" on), cfg/uwb_imu.yaml's (12 poses, an IMU prior per pose, RANGE + IMU messages) and cfg/uwb_twist.yaml's
(15 poses, an EdgeSE3 per pair, TWIST messages: the 6 x 6 inversion per window); 256 distinct windows tiled to the batch, numeric Jacobians.

Per shape and batch size, median of --reps with the spread (min .. max), the two cycles alternating (which goes first changes every rep):
  cycle_push         solve_resident, push_messages_resident_dev, solve_resident, synchronised                                 wall clock
  cycle_host_rows    solve_resident, download the poses, numpy rows (vectorised over the batch), to the device, slide_*_resident_dev,
                     solve_resident, synchronised                                                                             wall clock
  download / numpy_rows / to_device     of that: the three steps between the solve and the slide                                  wall clock
  build_launch       window_message_kernel alone (message_rows_dev)                     HIP events (loc_window_last_covariance_ms)
  slide_launch       the slide it feeds alone (uwb_only: the marginal pass + the re-pack)  HIP events
  solve_kernel_ms    the solve kernel alone on the slid batch                            HIP events (loc_window_timing_*)
  message_bytes / row_bytes   what the build must read per window (the message arrays under the mask) and what it writes (the rows of an
                     appended window with the scalars)
Every cycle starts from a fresh upload of the same batch (not timed).  uwb_only and uwb_imu must end on the same bits (asserted); the TWIST
rows of the host path come from numpy's sin / cos / inv, so uwb_twist reports the largest pose difference instead.  One JSON line per row.

    python tests/perf/bench_message_rows.py [--batches 65536,4096] [--reps 7] [--shapes uwb_only,uwb_imu,uwb_twist]
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
RANGE, IMU, LIDAR, TWIST = 1, 2, 4, 8
SHAPES = {"uwb_only": dict(T=10, se3=0, priors=1, chain3=True, kind=RANGE), "uwb_imu": dict(T=12, se3=0, priors=1, chain3=False, kind=RANGE | IMU),
          "uwb_twist": dict(T=15, se3=1, priors=0, chain3=False, kind=TWIST)}
from localization_amd.window import WindowBatch

TABLES = WindowBatch.TABLES
VMAX, OUTLIER = 5.0, 1.0


def _stats(xs):
    return {"median": round(float(np.median(xs)), 4), "min": round(float(min(xs)), 4), "max": round(float(max(xs)), 4)}


def _tile(a, B):
    return np.ascontiguousarray(np.concatenate([a] * -(-B // len(a)))[:B])


def _inv_rows(R, t):
    """Z^-1 rows of a batch: R [B][9] row-major, t [B][3] -> [B][12], the sums left to right"""
    Ri = R.reshape(-1, 3, 3).transpose(0, 2, 1).reshape(-1, 9)
    ti = np.stack([-((Ri[:, 3 * i] * t[:, 0] + Ri[:, 3 * i + 1] * t[:, 1]) + Ri[:, 3 * i + 2] * t[:, 2]) for i in range(3)], axis=1)
    return np.concatenate([Ri, ti], axis=1)


def numpy_rows(kind, T, x, anchors, antenna, m):
    """the rows of a batch of windows AT THEIR LAG (nv == T) from their newest solved poses x [B][12], vectorised: (new_pose, ranges, priors,
    se3, drop, appended) in the slides' layouts — the statement of tests/_message_rows_ref.py, operation for operation where numpy allows"""
    B, s = len(x), T - 1
    pose = x.copy()
    ok = np.ones(B, dtype=bool)
    rc, ri, rv = np.zeros(B, dtype=np.int32), np.zeros((B, 2, 2), dtype=np.int32), np.zeros((B, 2, 5))
    pc, pv = np.zeros(B, dtype=np.int32), np.zeros((B, 2, 18))
    sc, si, sv = np.zeros(B, dtype=np.int32), np.zeros((B, 1, 4), dtype=np.int32), np.zeros((B, 1, 48))
    if kind & RANGE:
        q = anchors[m["anchor"]]
        d = m["distance"].astype(np.float64)
        dx, dy, dz = (x[:, 9 + k] - q[:, k] for k in range(3))
        ok = ~(np.abs(np.sqrt((dx * dx + dy * dy) + dz * dz) - d) > OUTLIER)
        e = m["distance_err"].astype(np.float64)
        sd = VMAX * m["dt"] / 3
        ri[:, 0, 0] = s; ri[:, 0, 1] = -1 - m["anchor"]; ri[:, 1, 0] = s - 1; ri[:, 1, 1] = s
        rv[:, 0, 0] = d; rv[:, 0, 1] = 1.0 / (e * e); rv[:, 1, 1] = 1.0 / (sd * sd)
        rv[:, 0, 2:] = np.where((m["antenna"] > 0)[:, None], antenna[np.maximum(m["antenna"] - 1, 0)], 0.0)
        rc[:] = 2
        if kind & IMU:
            qx, qy, qz, qw = (m["imu"][:, k] for k in range(4))
            tx, ty, tz = 2 * qx, 2 * qy, 2 * qz
            twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * qw, ty * qw, tz * qw, tx * qx, ty * qx, tz * qx, ty * qy, tz * qy, tz * qz
            pose[:, :9] = np.stack([1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)], axis=1)
            pv[:, 0, :12] = _inv_rows(pose[:, :9], pose[:, 9:])
            pv[:, 0, 15:] = 1.0 / m["imu"][:, 4:7]
            pc[:] = 1
    else:   # TWIST
        tw, dt = m["twist"], m["dt"]
        hr, hp, hy = (tw[:, 3 + k] * dt * 0.5 for k in range(3))
        cy, sy, cp, sp, cr, sr = np.cos(hy), np.sin(hy), np.cos(hp), np.sin(hp), np.cos(hr), np.sin(hr)
        qx, qy, qz, qw = sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy
        n = 2.0 / (((qx * qx + qy * qy) + qz * qz) + qw * qw)
        xs, ys, zs = qx * n, qy * n, qz * n
        wx, wy, wz, xx, xy, xz, yy, yz, zz = qw * xs, qw * ys, qw * zs, qx * xs, qx * ys, qx * zs, qy * ys, qy * zs, qz * zs
        R = np.stack([1.0 - (yy + zz), xy - wz, xz + wy, xy + wz, 1.0 - (xx + zz), yz - wx, xz - wy, yz + wx, 1.0 - (xx + yy)], axis=1)
        sv[:, 0, :12] = _inv_rows(R, tw[:, :3] * dt[:, None])
        sv[:, 0, 12:] = np.linalg.inv((tw[:, 6:] * dt[:, None] * dt[:, None]).reshape(B, 6, 6)).reshape(B, 36)
        si[:, 0] = (s - 1, s, 1, 0)
        sc[:] = 1
    for c in (rc, pc, sc):
        c[~ok] = -1
    pose[~ok] = x[~ok]
    return pose, (rc, ri, rv), (pc, pv), (sc, si, sv), np.ones(B, dtype=np.int32), ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="65536,4096")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="uwb_only,uwb_imu,uwb_twist")
    args = ap.parse_args()
    import torch
    import localization_amd as la
    import _message_rows_ref as M
    import _slide_plain_ref as P
    dev = torch.device("cuda", 0)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    for shape in args.shapes.split(","):
        spec = SHAPES[shape]
        T, kind = spec["T"], spec["kind"]
        streams = [P.Stream(8800 + i, T + 1, 1, spec["priors"], spec["se3"]) for i in range(DISTINCT)]
        caps = P.caps_of(T, 1, spec["priors"], spec["se3"])
        base = P.window_batch(la, streams, [T] * DISTINCT, caps)
        if spec["chain3"]:
            base.poses[:, :, :9] = np.eye(3).reshape(9)
            base.r_val[:, :, 2:] = 0.0
            base.p_val[:, :, :9] = np.eye(3).reshape(9); base.p_val[:, :, 15:] = 0.0; base.p_val[:, :, 12:15] = 4.0
        rng = np.random.default_rng(8900)
        m0 = M.empty_messages(DISTINCT)
        for b in range(DISTINCT):
            M.fill_message(rng, m0, b, kind, base.poses[b, T - 1])
            if spec["chain3"]:
                m0["antenna"][b] = 0
        for B in (int(x) for x in args.batches.split(",")):
            wb = la.WindowBatch(B, *caps)
            for name in TABLES:
                getattr(wb, name)[:] = _tile(getattr(base, name), B)
            msgs = {k: _tile(v, B) for k, v in m0.items()}
            d_msgs = {k: (None if v is None else to(v)) for k, v in M.masked(msgs, kind).items()}
            message_bytes = sum(v[0].nbytes for k, v in M.masked(msgs, kind).items() if v is not None)
            row_bytes = 4 * 5 + 12 * 8 + (2 * (2 * 4 + 5 * 8) if kind & RANGE else 0) + (18 * 8 if kind & IMU else 0) + (4 * 4 + 48 * 8 if kind & TWIST else 0)
            d = la.WindowSolver(P.ANCH, B, *caps, jacobian="numeric")
            h = la.WindowSolver(P.ANCH, B, *caps, jacobian="numeric")
            for s in (d, h):
                s.set_option("resident_slide", 1)
                if spec["chain3"]:   # (the table the marginal carry makes is solved on wave3_lm_kernel, as in bench_resident_slide*.py)
                    s.set_option("prior_information_structured", 1)
                s.set_message_config(T, VMAX, OUTLIER, M.ANTENNA)
            verdict = torch.zeros(B, dtype=torch.int32, device=dev)
            admit = torch.zeros(B, dtype=torch.int32, device=dev)
            outs = dict(drop_oldest=torch.zeros(B, dtype=torch.int32, device=dev), new_pose=torch.zeros((B, 12), dtype=torch.float64, device=dev),
                        new_r_counts=torch.zeros(B, dtype=torch.int32, device=dev), new_r_idx=torch.zeros((B, 2, 2), dtype=torch.int32, device=dev),
                        new_r_val=torch.zeros((B, 2, 5), dtype=torch.float64, device=dev), new_p_counts=torch.zeros(B, dtype=torch.int32, device=dev),
                        new_p_val=torch.zeros((B, 2, 18), dtype=torch.float64, device=dev), new_s_counts=torch.zeros(B, dtype=torch.int32, device=dev),
                        new_s_idx=torch.zeros((B, 1, 4), dtype=torch.int32, device=dev), new_s_val=torch.zeros((B, 1, 48), dtype=torch.float64, device=dev))
            torch.cuda.synchronize()
            out_d, out_h, x = la.WindowBatch(B, *caps), la.WindowBatch(B, *caps), la.WindowBatch(B, *caps)
            t = {k: [] for k in ("cycle_push", "cycle_host_rows", "download", "numpy_rows", "to_device", "build_launch", "slide_launch", "solve_kernel_ms")}

            def push_cycle():
                d.upload(wb)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                d.solve_resident()
                d.push_messages_resident_dev(kind, d_msgs, verdict=verdict, admit=admit)
                d.solve_resident()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                slide_ms = d.last_covariance_ms()
                d.timing_begin(1)   # (not part of a cycle: the solve kernel alone, on the slid batch)
                d.solve_resident()
                solve_ms = d.timing_end()[1]
                d.message_rows_dev(kind, d_msgs, outs)   # (nor this: the build launch alone)
                torch.cuda.synchronize()
                return (t1 - t0) * 1e3, slide_ms, solve_ms, d.last_covariance_ms()

            def host_cycle():
                h.upload(wb)
                torch.cuda.synchronize()
                u0 = time.perf_counter()
                h.solve_resident()
                h.download(x)
                u1 = time.perf_counter()
                pose, ranges, priors, se3, drop, ok = numpy_rows(kind, T, x.poses[:, T - 1], P.ANCH, M.ANTENNA, msgs)
                u2 = time.perf_counter()
                t_pose, t_drop = to(pose), to(drop)
                t_ranges, t_priors, t_se3 = tuple(to(a) for a in ranges) + (2,), tuple(to(a) for a in priors) + (2,), tuple(to(a) for a in se3) + (1,)
                torch.cuda.synchronize()
                u3 = time.perf_counter()
                if spec["chain3"]:
                    h.slide_resident_dev(t_pose, t_ranges, t_priors, t_drop)
                else:
                    h.slide_plain_resident_dev(t_pose, t_ranges, t_priors, t_se3, t_drop)
                h.solve_resident()
                torch.cuda.synchronize()
                u4 = time.perf_counter()
                return (u4 - u0) * 1e3, (u1 - u0) * 1e3, (u2 - u1) * 1e3, (u3 - u2) * 1e3, ok

            for rep in range(args.reps + 1):   # (the first round warms both paths up: allocations, the first launches)
                if rep % 2:
                    hc, pc = host_cycle(), push_cycle()
                else:
                    pc, hc = push_cycle(), host_cycle()
                if rep == 0:
                    v, a = verdict.cpu().numpy(), admit.cpu().numpy()
                    assert ((v == 1) == hc[4]).all() and (a[v == 1] == 0).all() and (v == 1).sum() > B // 2, (np.bincount(v), np.bincount(a))
                    continue
                t["cycle_push"].append(pc[0]); t["slide_launch"].append(pc[1]); t["solve_kernel_ms"].append(pc[2]); t["build_launch"].append(pc[3])
                t["cycle_host_rows"].append(hc[0]); t["download"].append(hc[1]); t["numpy_rows"].append(hc[2]); t["to_device"].append(hc[3])
            d.download(out_d); h.download(out_h)
            diff = float(np.abs(out_d.poses - out_h.poses).max())
            same = out_d.poses.tobytes() == out_h.poses.tobytes() and out_d.result.tobytes() == out_h.result.tobytes()
            assert same or kind == TWIST, "the two cycles must end on the same bits"
            solve_kind = d.last_kernel_kind()
            d.close(); h.close()
            row = {"shape": shape, "windows": B, "poses": T, "reps": args.reps, "solve_kernel": solve_kind, "cycles_end_on_the_same_bits": same,
                   "largest_pose_difference": diff, "appended": int(hc[4].sum()), "message_bytes_per_window": int(message_bytes), "row_bytes_per_window": int(row_bytes)}
            row.update({k: _stats(v) for k, v in t.items()})
            row["host_rows_over_push"] = round(row["cycle_host_rows"]["median"] / row["cycle_push"]["median"], 2)
            row["build_launch_over_slide_launch"] = round(row["build_launch"]["median"] / row["slide_launch"]["median"], 3)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
