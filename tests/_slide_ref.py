"""Test helper: the rule of the resident fixed-lag slide (loc_window_slide_resident; DESIGN.md §2, "The resident slide") stated in numpy on a
WindowBatch — what tests/test_resident_slide_cpu.py holds the host's index function to and tests/test_gpu_resident_slide.py the device
tables, bit for bit.  The marginal prior of slot 0 is an INPUT here (slot [B], prior [B][48]: loc_window_marginal_prior_host's, or
tests/_dense_prior_ref.marginal_ref's): this file moves rows and computes nothing.

new_rows() builds the appended pose and factors of tests/_fixed_lag.Chain windows."""
import numpy as np

import _fixed_lag as F


def slide_ref(la, wb, slot, prior, new_pose, new_ranges=None, new_priors=None, drop_oldest=None):
    """The batch after the slide of wb (poses: the solved estimates x).  slot / prior: the marginal of slot 0 of every window (read for the
    windows that drop); new_pose [B][12]; new_ranges (counts [B], r_idx [B][n][2], r_val [B][n][5]) in the new numbering; new_priors (counts
    [B], p_val [B][n][18]) on the new slot; drop_oldest [B] (None: every window drops).  The result always carries p_info: wb's, or
    diag(p_val[12..17]) of every prior that had none."""
    B = wb.B
    nv_max, nr_max, np_max, ns_max = wb.caps
    out = la.WindowBatch(B, *wb.caps)
    out.p_info = np.zeros((B, max(np_max, 1), 36))
    old_info = getattr(wb, "p_info", None)
    new_pose = np.asarray(new_pose, dtype=float).reshape(B, 12)
    for b in range(B):
        nv, nr, npr, _ = (int(x) for x in wb.counts[b])
        assert nv >= 1
        drop = True if drop_oldest is None else bool(np.broadcast_to(drop_oldest, (B,))[b])
        info = lambda e: old_info[b, e].copy() if old_info is not None else np.diag(wb.p_val[b, e, 12:18]).reshape(36)
        ranges, priors = [], []   # (idx, val), (idx, val, info)
        if drop:
            if slot[b] >= 0:   # the carried prior: row 0 on the new slot 0 (the zero row of a singular marginal is a row)
                val = np.concatenate([prior[b, :12], prior[b, 12:].reshape(6, 6).diagonal()])
                priors.append((int(slot[b]) - 1, val, prior[b, 12:].copy()))
            for e in range(nr):
                v0, v1 = (int(x) for x in wb.r_idx[b, e])
                if v0 != 0 and v1 != 0:
                    ranges.append(((v0 - 1, v1 - 1 if v1 > 0 else v1), wb.r_val[b, e].copy()))
            for e in range(npr):
                if int(wb.p_idx[b, e]) != 0:
                    priors.append((int(wb.p_idx[b, e]) - 1, wb.p_val[b, e].copy(), info(e)))
            poses = wb.poses[b, 1:nv]
        else:
            ranges = [(tuple(int(x) for x in wb.r_idx[b, e]), wb.r_val[b, e].copy()) for e in range(nr)]
            priors = [(int(wb.p_idx[b, e]), wb.p_val[b, e].copy(), info(e)) for e in range(npr)]
            poses = wb.poses[b, :nv]
        s = len(poses)   # the new slot
        if new_ranges is not None:
            for e in range(int(new_ranges[0][b])):
                ranges.append((tuple(int(x) for x in new_ranges[1][b][e]), np.asarray(new_ranges[2][b][e], dtype=float).copy()))
        if new_priors is not None:
            for e in range(int(new_priors[0][b])):
                val = np.asarray(new_priors[1][b][e], dtype=float).copy()
                priors.append((s, val, np.diag(val[12:18]).reshape(36)))
        assert s + 1 <= nv_max and len(ranges) <= nr_max and len(priors) <= np_max
        out.counts[b] = (s + 1, len(ranges), len(priors), 0)
        out.poses[b, :s] = poses
        out.poses[b, s] = new_pose[b]
        for e, (ix, val) in enumerate(ranges):
            out.r_idx[b, e] = ix; out.r_val[b, e] = val
        for e, (v, val, W) in enumerate(priors):
            out.p_idx[b, e] = v; out.p_val[b, e] = val; out.p_info[b, e] = W
    return out


def new_rows(chains, pose_index, new_slot, doubled=()):
    """(new_pose [B][12], new_ranges) for pose pose_index[b] of chains[b] appended as slot new_slot[b]: the chain's estimate, its anchor
    ranges, and the smoothness edge to the slot before it (stored (s, s - 1) for odd s, as tests/_fixed_lag.add_chain_poses does; none for
    s = 0).  doubled: windows that get a second one the other way round."""
    B = len(chains)
    nmax = F.NA_MAX + 2
    pose = np.zeros((B, 12)); pose[:, 0] = pose[:, 4] = pose[:, 8] = 1.0
    counts = np.zeros(B, dtype=np.int32)
    r_idx = np.zeros((B, nmax, 2), dtype=np.int32)
    r_val = np.zeros((B, nmax, 5))
    for b, ch in enumerate(chains):
        k, s = int(pose_index[b]), int(new_slot[b])
        pose[b, 9:] = ch.est[k]
        rows = [((s, -1 - a), (d, F.RANGE_INFO, 0, 0, 0)) for a, d in zip(ch.which[k], ch.meas[k])]
        if s:
            rows.append(((s, s - 1) if s % 2 else (s - 1, s), (0.0, F.SMOOTH_INFO, 0, 0, 0)))
            if b in doubled:
                rows.append(((s - 1, s) if s % 2 else (s, s - 1), (0.0, 0.5 * F.SMOOTH_INFO, 0, 0, 0)))
        counts[b] = len(rows)
        for e, (ix, val) in enumerate(rows):
            r_idx[b, e] = ix; r_val[b, e] = val
    return pose, (counts, r_idx, r_val)


def assert_same_tables(got, ref, what=""):
    """counts, every index and value table and p_info of two batches, bitwise, on the used rows (rows beyond the counts are not compared)"""
    assert np.array_equal(got.counts, ref.counts), (what, got.counts, ref.counts)
    assert got.p_info is not None and ref.p_info is not None, what
    for b in range(ref.B):
        nv, nr, npr, _ = (int(x) for x in ref.counts[b])
        for name, n in (("poses", nv), ("r_idx", nr), ("r_val", nr), ("p_idx", npr), ("p_val", npr), ("p_info", npr)):
            x, y = getattr(got, name)[b, :n], getattr(ref, name)[b, :n]
            assert x.tobytes() == y.tobytes(), (what, name, b, x, y)


# ---- the inputs of the slide tests: name -> eight windows of tests/_fixed_lag.Chain ----------------------------------------------------------------
NP_MAX = 4
Z_INFO = np.array([0, 0, 1 / 0.05, 0, 0, 0.0])
CASES = {
    "plain": dict(T=[6] * 8),
    "doubled": dict(T=[6] * 8, doubled=(1,)),                         # a second smoothness edge on (0, 1), the other way round
    "zprior": dict(T=[6] * 8, zprior=(0, 2), new_prior=True),         # a z prior on slot 0 (removed) and on slot 2 (kept, renumbered, densified)
    "table": dict(T=[6] * 8, fullprior=True),                         # the caller set a table of rank 1 .. 3 matrices beforehand
    "missing": dict(T=[6] * 8, missing_even=True),                    # no link (0, 1) in every other window: slot -1, no row
    "one_range": dict(T=[6] * 8, one_range=(2, 5)),                   # slot 0 keeps one anchor range: LOC_ERR_SINGULAR, the zero row is inserted
    "ragged": dict(T=[1, 2, 4, 6, 1, 2, 4, 6], drop=[1, 0, 1, 1, 0, 1, 0, 1], nv_max=9),
    "long": dict(T=[20] * 8, na=4, zprior=(3, 7, 11)),                # 99 range rows; the carried prior shifts three kept priors
}
SEED = {name: 8200 + 10 * k for k, name in enumerate(CASES)}


def caps_for(nv_max):
    return nv_max, nv_max * F.NA_MAX + 2 * (nv_max - 1), NP_MAX, 0


def case_batch(la, name):
    """(batch, chains, spec) of a slide case; spec["drop"]: drop_oldest of every slide (None: all), spec["consumed"]: chain poses used so far"""
    spec = dict(CASES[name])
    T = spec["T"]
    chains = [F.Chain(SEED[name] + i, T[i] + 6, spec.get("na", 3 + i % 3)) for i in range(8)]
    wb = la.WindowBatch(8, *caps_for(spec.get("nv_max", max(T))))
    rng = np.random.default_rng(SEED[name] + 5)
    for i, ch in enumerate(chains):
        F.add_chain_poses(wb, i, ch, 0, T[i], doubled=spec.get("doubled", ()), missing=(1,) if spec.get("missing_even") and i % 2 == 0 else (),
                          keep_ranges={0: 1} if i in spec.get("one_range", ()) else None)
        for s in spec.get("zprior", ()):
            wb.add_prior(i, s, np.array([ch.est[s, 0], ch.est[s, 1], ch.truth[s, 2] + rng.normal(0, 0.02)]), np.eye(3), Z_INFO)
        if spec.get("fullprior"):
            A = rng.normal(size=(3, 1 + i % 3))
            info = np.zeros((6, 6)); info[:3, :3] = 40.0 * (A @ A.T)
            s = 0 if i % 2 == 0 else 3
            wb.add_prior(i, s, ch.truth[s] + rng.normal(0, 0.05, 3), np.eye(3), info=info)
    spec["consumed"] = np.array(T)
    spec["drop"] = None if "drop" not in spec else np.array(spec["drop"], dtype=np.int32)
    return wb, chains, spec


def next_inputs(wb, chains, spec):
    """(new_pose, new_ranges, new_priors, drop_oldest) of the next slide of a case at batch wb (its counts), advancing spec["consumed"]"""
    drop = spec["drop"]
    nv = wb.counts[:, 0].astype(int)
    slot = nv - (1 if drop is None else (drop != 0).astype(int))
    pose, ranges = new_rows(chains, spec["consumed"], slot)
    priors = None
    if spec.get("new_prior"):   # a z prior on the new pose of the odd windows
        pc = np.array([i % 2 for i in range(8)], dtype=np.int32)
        pv = np.zeros((8, 1, 18)); pv[:, 0, 0] = pv[:, 0, 4] = pv[:, 0, 8] = 1.0
        for i, ch in enumerate(chains):
            pv[i, 0, 9:12] = -np.array([ch.est[spec["consumed"][i], 0], ch.est[spec["consumed"][i], 1], ch.truth[spec["consumed"][i], 2]])
            pv[i, 0, 12:] = Z_INFO
        priors = (pc, pv)
    spec["consumed"] = spec["consumed"] + 1
    return pose, ranges, priors, drop
