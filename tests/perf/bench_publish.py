#!/usr/bin/env python3
"""What the publish step of a resident batch costs and what it saves (loc_window_publish_resident, loc_window_path_resident),
on two shapes at two batch sizes:
  uwb_only   translation-only chain windows of T = 10 poses (tests/_slide_plain_ref.py's streams without anything that turns a pose)
  uwb_twist  6-DoF chain windows of T = 15 poses with an EdgeSE3 per consecutive pair and two priors per pose
64 distinct windows, tiled.  Both sides of every comparison run in this process, alternated; medians of --reps with the spread (min .. max).

  (a) launches   publish_ms, path_ms (first = 0, count = T): HIP events around the launch (loc_window_last_covariance_ms), beside solve_ms,
                 the resident solve they follow (loc_window_timing_*)
  (b) one cycle  resident_ms: solve, publish, copy flags + realtime + optimized to page-locked host memory, one synchronisation;
                 download_ms: solve, loc_window_download, the same records formed in numpy.  Host clock around work that ends in a
                 synchronisation.  The two sides' records are compared bit for bit once (records_equal).
  (c) K queued   resident_ms: K cycles of (push_messages, solve, publish + the three copies) on one stream, ONE synchronisation at the end;
                 download_ms: the same K cycles with a download and the numpy records after every solve.  The batch is uploaded and solved
                 afresh before each side (not timed).
and the bytes each side of (b) moves across the link per cycle.  Prints one JSON line per (part, shape, batch size).

    python tests/perf/bench_publish.py [--reps 7] [--sizes 4096,65536] [--cycles 8] [--parts abc]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

BASE = 64   # distinct windows
SHAPES = {"uwb_only": dict(T=10, priors=1, se3=0, chain3=True), "uwb_twist": dict(T=15, priors=2, se3=1, chain3=False)}


def _stats(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4)}


def _base_batch(la, P, name):
    f = SHAPES[name]
    T = f["T"]
    streams = [P.Stream(9700 + i, T + 1, 1, f["priors"], f["se3"]) for i in range(BASE)]
    wb = P.window_batch(la, streams, np.full(BASE, T), P.caps_of(T, 1, f["priors"], f["se3"]))
    if f["chain3"]:
        wb.poses[:, :, :9] = np.eye(3).reshape(9)
        wb.r_val[:, :, 2:] = 0.0
        wb.p_val[:, :, :9] = np.eye(3).reshape(9); wb.p_val[:, :, 15:] = 0.0; wb.p_val[:, :, 12:15] = 4.0
    return wb


def _messages(M, name, base, K, B):
    """K cycles of one message per window (uwb_only: RANGE; uwb_twist: RANGE, TWIST alternating), made for the 64 windows and tiled"""
    f = SHAPES[name]
    pick = np.arange(B) % BASE
    out = []
    for k in range(K):
        kind = M.RANGE if f["chain3"] or k % 2 == 0 else M.TWIST
        rng = np.random.default_rng(9800 + k)
        msgs = M.empty_messages(BASE)
        for b in range(BASE):
            M.fill_message(rng, msgs, b, kind, base.poses[b, f["T"] - 1], turning=False)
            if f["chain3"]:
                msgs["antenna"][b] = 0
        out.append({key: v[pick] for key, v in msgs.items()})
    return out, (M.RANGE if f["chain3"] else M.RANGE | M.TWIST)


def records_numpy(p):
    """the 7-double records of poses [n][12], vectorised: Eigen's Quaternion(Matrix3) and the flip to w >= 0 (tests/_publish_ref.py's statement)"""
    m = lambda r, c: p[:, 3 * r + c]
    with np.errstate(all="ignore"):
        tr = m(0, 0) + m(1, 1) + m(2, 2)
        i = np.where(m(1, 1) > m(0, 0), 1, 0)
        i = np.where(m(2, 2) > np.where(i == 1, m(1, 1), m(0, 0)), 2, i)
        q = np.empty((len(p), 4))   # x, y, z, w
        t = np.sqrt(tr + 1.0)
        w0 = 0.5 * t
        t = 0.5 / t
        q[:, 0] = (m(2, 1) - m(1, 2)) * t; q[:, 1] = (m(0, 2) - m(2, 0)) * t; q[:, 2] = (m(1, 0) - m(0, 1)) * t; q[:, 3] = w0
        for a in range(3):
            b, c = (a + 1) % 3, (a + 2) % 3
            sel = (~(tr > 0)) & (i == a)
            if not sel.any():
                continue
            t = np.sqrt(m(a, a) - m(b, b) - m(c, c) + 1.0)
            qa = 0.5 * t
            t = 0.5 / t
            q[sel, a] = qa[sel]
            q[sel, 3] = ((m(c, b) - m(b, c)) * t)[sel]
            q[sel, b] = ((m(b, a) + m(a, b)) * t)[sel]
            q[sel, c] = ((m(c, a) + m(a, c)) * t)[sel]
        q[q[:, 3] < 0] *= -1.0
    return np.concatenate([p[:, 9:12], q], axis=1)


def publish_numpy(poses, result, thr, T):
    """flags, realtime, optimized of full windows (nv = T) from downloaded poses and result"""
    pub = result[:, 0] < thr
    flags = pub.astype(np.int32) | 2
    return flags, records_numpy(poses[:, T - 1]), records_numpy(poses[:, T // 2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", default="4096,65536")
    ap.add_argument("--cycles", type=int, default=8)
    ap.add_argument("--parts", default="abc")
    args = ap.parse_args()
    import torch
    import localization_amd as la
    import _message_rows_ref as M
    import _slide_plain_ref as P
    dev = torch.device("cuda", 0)
    for name in SHAPES:
        T = SHAPES[name]["T"]
        base = _base_batch(la, P, name)
        for B in (int(x) for x in args.sizes.split(",")):
            wb = base.tile(B)
            s = la.WindowSolver(P.ANCH, B, *wb.caps, jacobian="numeric")
            s.set_option("resident_slide", 1)
            s.set_message_config(T, 5.0, 1.0, M.ANTENNA)
            host = la.WindowBatch(B, *wb.caps)
            d = dict(flags=torch.zeros(B, dtype=torch.int32, device=dev), realtime=torch.zeros((B, 7), dtype=torch.float64, device=dev),
                     optimized=torch.zeros((B, 7), dtype=torch.float64, device=dev), n=torch.zeros(1, dtype=torch.int32, device=dev))
            pinned = {k: torch.empty_like(d[k], device="cpu").pin_memory() for k in ("flags", "realtime", "optimized")}
            path, present = torch.zeros((B, T, 7), dtype=torch.float64, device=dev), torch.zeros((B, T), dtype=torch.int32, device=dev)
            st = torch.cuda.Stream()
            s.upload(wb); s.solve_resident(); s.download(host)
            thr = float(np.median(host.result[:, 0]))
            common = {"shape": name, "windows": B, "poses": T, "reps": args.reps, "threshold": thr}

            def resident_cycle():
                s.solve_resident(stream=st.cuda_stream)
                s.publish_resident(thr, T, d["flags"], d["realtime"], d["optimized"], None, d["n"], stream=st)
                with torch.cuda.stream(st):
                    for k, h in pinned.items():
                        h.copy_(d[k], non_blocking=True)

            def download_cycle():
                s.solve_resident(stream=st.cuda_stream)
                s.download(host)
                return publish_numpy(host.poses, host.result, thr, T)

            torch.cuda.synchronize()
            if "a" in args.parts:
                t = {"solve_ms": [], "publish_ms": [], "path_ms": []}
                for rep in range(args.reps + 1):   # (the first round warms up)
                    s.timing_begin(1)
                    s.solve_resident()
                    solve_ms = s.timing_end()[2]
                    s.publish_resident(thr, T, d["flags"], d["realtime"], d["optimized"], None, d["n"])
                    publish_ms = s.last_covariance_ms()
                    s.path_resident(T, path, present)
                    path_ms = s.last_covariance_ms()
                    if rep:
                        t["solve_ms"].append(solve_ms); t["publish_ms"].append(publish_ms); t["path_ms"].append(path_ms)
                torch.cuda.synchronize()
                row = dict(common, part="a", solve_kernel=s.last_kernel_kind(), n_published=int(d["n"].item()))
                row.update({k: _stats(v) for k, v in t.items()})
                row["publish_bytes"] = B * (4 + 8 + 2 * 96 + 4 + 2 * 56); row["path_bytes"] = B * (4 + T * (96 + 56 + 4))
                row["publish_over_solve"] = round(row["publish_ms"]["median"] / row["solve_ms"]["median"], 4)
                row["path_over_solve"] = round(row["path_ms"]["median"] / row["solve_ms"]["median"], 4)
                print(json.dumps(row), flush=True)
            if "b" in args.parts:
                t = {"resident_ms": [], "download_ms": []}
                equal = None
                for rep in range(args.reps + 1):
                    t0 = time.perf_counter()
                    resident_cycle(); st.synchronize()
                    t1 = time.perf_counter()
                    flags, rt, opt = download_cycle()
                    t2 = time.perf_counter()
                    if rep:
                        t["resident_ms"].append((t1 - t0) * 1e3); t["download_ms"].append((t2 - t1) * 1e3)
                    else:
                        pubd = flags & 1 == 1
                        equal = bool((pinned["flags"].numpy() == flags).all() and pinned["realtime"].numpy()[pubd].tobytes() == rt[pubd].tobytes()
                                     and pinned["optimized"].numpy()[pubd].tobytes() == opt[pubd].tobytes())
                row = dict(common, part="b", records_equal=equal)
                row.update({k: _stats(v) for k, v in t.items()})
                row["resident_link_bytes"] = B * (4 + 2 * 56); row["download_link_bytes"] = B * (T * 96 + 64)
                row["download_over_resident"] = round(row["download_ms"]["median"] / row["resident_ms"]["median"], 3)
                print(json.dumps(row), flush=True)
            if "c" in args.parts:
                K = args.cycles
                cycles, mask = _messages(M, name, base, K, B)
                dm = [{k: (None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(dev)) for k, v in M.masked(c, mask).items()} for c in cycles]
                t = {"resident_ms": [], "download_ms": []}
                for rep in range(args.reps + 1):
                    for side in ("resident_ms", "download_ms"):
                        s.upload(wb); s.solve_resident()
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        for k in range(K):
                            s.push_messages_resident_dev(mask, dm[k], stream=st)
                            if side == "resident_ms":
                                resident_cycle()
                            else:
                                download_cycle()
                        st.synchronize()
                        if rep:
                            t[side].append((time.perf_counter() - t0) * 1e3)
                row = dict(common, part="c", cycles=K, solve_kernel=s.last_kernel_kind())
                row.update({k: _stats(v) for k, v in t.items()})
                row["download_over_resident"] = round(row["download_ms"]["median"] / row["resident_ms"]["median"], 3)
                print(json.dumps(row), flush=True)
            s.close()


if __name__ == "__main__":
    main()
