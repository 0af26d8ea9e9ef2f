"""Rows from raw messages on the device (loc_window_set_message_config, loc_window_message_rows_dev, loc_window_push_messages_resident_dev;
window_message_kernel.hip; DESIGN.md §2, "Rows from raw messages").  The yardstick is the statement written from the reference
(tests/_message_rows_ref.py), BIT FOR BIT on all eleven output arrays; only the twelve Z^-1 entries of a TWIST row with a non-zero angular
rate are held to M.TWIST_BOUND (sin and cos).  The pushes are held, bit for bit, to a second handle driven step by step through download ->
numpy rows -> the existing slide_*_resident_dev call.

Smallest shapes: 130 windows (no multiple of 4, 8 or 64: a ragged last workgroup), trajectory_length 4 on nv_max 5, four anchors, windows of
1 to 4 poses mixed in one batch.  Each family is built and solved once and shared (_family); torch copies on ITS stream and the handle's
stream does not wait for it: every test synchronises before it hands pointers over."""
import functools

import numpy as np
import pytest

import _message_rows_ref as M
import _slide_plain_ref as P

pytestmark = pytest.mark.gpu

B, T, NV_MAX = 130, 4, 5
ALL = M.RANGE | M.IMU | M.LIDAR | M.TWIST
LOC_ERR_INVALID = -1
# family -> priors per pose, EdgeSE3 per pair, translation-only, the kinds of three consecutive cycles, kinds_mask, the solve kernel's verdict family
FAMILIES = {
    "uwb_only": dict(priors=1, se3=0, chain3=True, kinds=(M.RANGE,) * 3, mask=M.RANGE),
    "uwb_imu": dict(priors=1, se3=0, chain3=False, kinds=(M.RANGE | M.IMU,) * 3, mask=M.RANGE | M.IMU),
    "uwb_imu_lidar": dict(priors=2, se3=0, chain3=False, kinds=(M.RANGE | M.IMU | M.LIDAR,) * 3, mask=M.RANGE | M.IMU | M.LIDAR),
    "uwb_twist": dict(priors=2, se3=1, chain3=False, kinds=(M.RANGE, M.TWIST, M.RANGE), mask=M.RANGE | M.TWIST),
}
KERNELS = {"uwb_only": ("chain3_lm_kernel", "wave3_lm_kernel"), "uwb_imu": ("wave6_lm_kernel",), "uwb_imu_lidar": ("wave6_lm_kernel",),
           "uwb_twist": ("wave6_lm_kernel<SE3>",)}


def _config(s, cfg):
    s.set_message_config(cfg.T, cfg.vmax, cfg.outlier, cfg.antenna if len(cfg.antenna) else None)


def _batch(la, name, nvs=None, seed=0):
    """the family's windows: window i has nvs[i] poses (default 1, 2, 3, 4, 1, ...)"""
    f = FAMILIES[name]
    nvs = (np.arange(B) % T) + 1 if nvs is None else np.asarray(nvs)
    streams = [P.Stream(7100 + 1000 * seed + i, NV_MAX + 1, 1, f["priors"], f["se3"]) for i in range(len(nvs))]
    wb = P.window_batch(la, streams, nvs, P.caps_of(NV_MAX, 1, f["priors"], f["se3"]))
    if f["chain3"]:   # nothing that turns a pose: identity rotations, no lever arm, translation information only
        wb.poses[:, :, :9] = np.eye(3).reshape(9)
        wb.r_val[:, :, 2:] = 0.0
        wb.p_val[:, :, :9] = np.eye(3).reshape(9); wb.p_val[:, :, 15:] = 0.0; wb.p_val[:, :, 12:15] = 4.0
    return wb


def _solver(la, wb):
    s = la.WindowSolver(P.ANCH, wb.B, *wb.caps, jacobian="analytic")
    s.set_option("resident_slide", 1)
    return s


def _messages(name, cycle, wb, seed, turning=False, none_every=0):
    """one message per window for a cycle of the family, plausible for the windows' newest poses (as uploaded)"""
    f = FAMILIES[name]
    rng = np.random.default_rng(M.RANDOM_SEED + 100 * seed + cycle)
    msgs = M.empty_messages(wb.B)
    for b in range(wb.B):
        nv = max(int(wb.counts[b, 0]), 1)
        M.fill_message(rng, msgs, b, f["kinds"][cycle], wb.poses[b, nv - 1], turning=turning)
        if f["chain3"]:
            msgs["antenna"][b] = 0
        if none_every and b % none_every == 3:
            msgs["kind"][b] = 0
    return msgs


def _dev(arrays):
    import torch
    d = torch.device("cuda", 0)
    return {k: (None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(d)) for k, v in arrays.items()}


def _outputs(n):
    """the eleven output arrays, poisoned"""
    import torch
    d = torch.device("cuda", 0)
    i = lambda *shape: torch.full(shape, M.POISON_I, dtype=torch.int32, device=d)
    f = lambda *shape: torch.full(shape, M.POISON_D, dtype=torch.float64, device=d)
    return dict(drop_oldest=i(n), new_pose=f(n, 12), new_r_counts=i(n), new_r_idx=i(n, 2, 2), new_r_val=f(n, 2, 5), new_p_counts=i(n), new_p_val=f(n, 2, 18),
                new_s_counts=i(n), new_s_idx=i(n, 1, 4), new_s_val=f(n, 1, 48), verdict=i(n))


def _records(out):
    """the device outputs as the helper's RECORD array"""
    import torch
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in out.items()}
    n = len(h["verdict"])
    rec = np.zeros(n, dtype=M.RECORD)
    for f, k in (("drop", "drop_oldest"), ("nr", "new_r_counts"), ("np", "new_p_counts"), ("ns", "new_s_counts"), ("verdict", "verdict"), ("pose", "new_pose")):
        rec[f] = h[k]
    for f, k in (("r_idx", "new_r_idx"), ("s_idx", "new_s_idx"), ("r_val", "new_r_val"), ("p_val", "new_p_val"), ("s_val", "new_s_val")):
        rec[f] = h[k].reshape(n, -1)
    return rec


def _solved(la, s):
    wb = la.WindowBatch(s._resident, *s.caps)
    s.download(wb)
    return wb


def _newest(counts, poses):
    nv = counts[:, 0].astype(int)
    return nv, poses[np.arange(len(nv)), np.maximum(nv - 1, 0)]


def _statement(cfg, mask, counts, poses, msgs):
    nv, x = _newest(counts, poses)
    return M.batch_rows(cfg, mask, nv, x, P.ANCH, M.masked(msgs, mask))


def _build(s, mask, msgs, stream=None):
    import torch
    dm, out = _dev(M.masked(msgs, mask)), _outputs(len(msgs["kind"]))
    torch.cuda.synchronize()
    s.message_rows_dev(mask, dm, out, stream=stream)
    return _records(out)


@functools.lru_cache(maxsize=None)
def _family(name):
    """(solver, the uploaded batch, its solved poses): uploaded, configured and solved once"""
    import localization_amd as la
    wb = _batch(la, name)
    s = _solver(la, wb)
    s.upload(wb); s.solve_resident()
    kind = s.last_kernel_kind()
    _config(s, M.Config(T))
    return s, wb, _solved(la, s).poses.copy(), kind


# ---- 1. build only --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FAMILIES))
def test_build_only_bit_for_bit(gpu, name):
    s, wb, poses, kind = _family(name)
    assert kind in KERNELS[name], kind
    f = FAMILIES[name]
    worst = 0.0
    for cycle, turning in ((0, False), (1, True)):
        msgs = _messages(name, cycle, wb, seed=1, turning=turning, none_every=9)
        _config(s, M.Config(T))
        got = _build(s, f["mask"], msgs)
        want = _statement(M.Config(T), f["mask"], wb.counts, poses, msgs)
        worst = max(worst, M.assert_same_records(got, want, msgs, f"{name} cycle {cycle}"))   # (the poisoned rows beyond the counts among them)
        seen = np.bincount(want["verdict"], minlength=5)
        assert seen[M.APPENDED] > B // 2 and seen[M.NONE] > 0, seen
    print(f"{name}: largest |Z^-1 deviation| of a turning TWIST row: {worst:.3e} (measured {M.TWIST_MEASURED:.3e}, bound {M.TWIST_BOUND:.3e})")
    if name == "uwb_twist":
        assert (want["ns"] == 1).sum() > B // 2


def test_random_twist_rows_within_the_measured_bound(gpu):
    """the random TWIST windows the bound was measured on (M.RANDOM_SEED), and every other kind, under the mask of all four bits"""
    import localization_amd as la
    s, wb, poses, _ = _family("uwb_twist")
    rng = np.random.default_rng(M.RANDOM_SEED)
    nv, _ = _newest(wb.counts, poses)
    msgs = M.empty_messages(B)
    for b in range(B):
        M.fill_message(rng, msgs, b, int(rng.choice(M.LEGAL_KINDS + (M.TWIST, M.TWIST))), poses[b, nv[b] - 1])
    got = _build(s, ALL, msgs)
    want = _statement(M.Config(T), ALL, wb.counts, poses, msgs)
    worst = M.assert_same_records(got, want, msgs, "random")
    print(f"random: {int((want['ns'] == 1).sum())} TWIST rows, largest |Z^-1 deviation| {worst:.3e} (bound {M.TWIST_BOUND:.3e})")
    assert (want["ns"] == 1).sum() >= 40
    for seed in M.TWIST_SEEDS:   # the batches M.TWIST_MEASURED was measured on: a TWIST message for every window
        rng = np.random.default_rng(seed)
        for b in range(B):
            M.fill_message(rng, msgs, b, M.TWIST, poses[b, nv[b] - 1])
        got = _build(s, ALL, msgs)
        want = _statement(M.Config(T), ALL, wb.counts, poses, msgs)
        worst = max(worst, M.assert_same_records(got, want, msgs, f"twist {seed}"))
    print(f"TWIST_SEEDS: largest |Z^-1 deviation| {worst:.17g} (measured {M.TWIST_MEASURED:.17g}, bound {M.TWIST_BOUND:.3e})")


# ---- 2. the gate ------------------------------------------------------------------------------------------------------------------------------------------
def test_gate_decisions(gpu):
    s, wb, poses, _ = _family("uwb_imu")
    nv, x = _newest(wb.counts, poses)
    rng = np.random.default_rng(M.RANDOM_SEED + 7)
    msgs = M.empty_messages(B)
    outlier = 0.7
    lag = np.flatnonzero(nv == T)
    for b in range(B):
        M.fill_message(rng, msgs, b, M.RANGE | M.IMU, x[b])
        cases = M.gate_cases(x[b], P.ANCH, int(msgs["anchor"][b]), outlier)
        msgs["distance"][b] = cases[(b // T) % len(cases)][0]   # (the windows at their lag are every fourth: all six cases reach them)
    # one window at its lag with |est - d| == distance_outlier exactly (accepted): the configuration takes ITS difference as the threshold
    b0 = int(lag[0])
    exact = abs(M.estimate(x[b0], P.ANCH[int(msgs["anchor"][b0])]) - float(msgs["distance"][b0]))
    try:
        for cfg in (M.Config(T, outlier=outlier), M.Config(T, outlier=exact), M.Config(T, outlier=float(np.nextafter(exact, 0.0))), M.Config(T, outlier=0.0)):
            _config(s, cfg)
            got = _build(s, M.RANGE | M.IMU, msgs)
            want = _statement(cfg, M.RANGE | M.IMU, wb.counts, poses, msgs)
            assert got["verdict"].tolist() == want["verdict"].tolist(), cfg.outlier
            M.assert_same_records(got, want, msgs, f"gate {cfg.outlier}")
            rej = want["verdict"] == M.REJECTED
            if cfg.outlier == outlier:
                assert rej[lag].sum() >= len(lag) // 3 and (~rej[lag]).sum() >= len(lag) // 3 and not rej[nv < T].any()
            elif cfg.outlier == exact:
                assert want["verdict"][b0] == M.APPENDED
            elif cfg.outlier > 0:
                assert want["verdict"][b0] == M.REJECTED
            else:
                assert not rej.any()
    finally:
        _config(s, M.Config(T))


# ---- 3. queued cycles -------------------------------------------------------------------------------------------------------------------------------------
def _slide_with_rows(s, name, rec, stream=None):
    """the existing slide of the family's verdict, fed the statement's rows from device copies"""
    import torch
    n = len(rec)
    d = _dev(dict(pose=rec["pose"], drop=rec["drop"], rc=rec["nr"], ri=rec["r_idx"].reshape(n, 2, 2), rv=rec["r_val"].reshape(n, 2, 5), pc=rec["np"],
                  pv=rec["p_val"].reshape(n, 2, 18), sc=rec["ns"], si=rec["s_idx"].reshape(n, 1, 4), sv=rec["s_val"].reshape(n, 1, 48)))
    torch.cuda.synchronize()
    if FAMILIES[name]["chain3"]:
        s.slide_resident_dev(d["pose"], (d["rc"], d["ri"], d["rv"], 2), (d["pc"], d["pv"], 2), d["drop"], stream=stream)
    else:
        s.slide_plain_resident_dev(d["pose"], (d["rc"], d["ri"], d["rv"], 2), (d["pc"], d["pv"], 2), (d["sc"], d["si"], d["sv"], 1), d["drop"], stream=stream)
    return d


def _same_batches(a, b, what):
    P.assert_same_tables(a, b, what)
    assert (a.p_info is None) == (b.p_info is None), what
    if a.p_info is not None:
        for w in range(a.B):
            n = int(a.counts[w, 2])
            assert a.p_info[w, :n].tobytes() == b.p_info[w, :n].tobytes(), (what, "p_info", w)


@pytest.mark.parametrize("name", ["uwb_only", "uwb_imu", "uwb_twist"])
def test_three_queued_cycles(gpu, name):
    import torch
    import localization_amd as la
    f = FAMILIES[name]
    wb = _batch(la, name, seed=3)
    cfg = M.Config(T)
    cycles = [_messages(name, k, wb, seed=3, none_every=11) for k in range(3)]
    a, r = _solver(la, wb), _solver(la, wb)
    for s in (a, r):
        s.upload(wb); _config(s, cfg)
    # the handle under test: everything queued on one stream, no host call that waits in between
    dm = [_dev(M.masked(m, f["mask"])) for m in cycles]
    verdicts = [torch.full((B,), M.POISON_I, dtype=torch.int32, device="cuda") for _ in cycles]
    admits = [torch.full((B,), M.POISON_I, dtype=torch.int32, device="cuda") for _ in cycles]
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    for k in range(3):
        a.solve_resident(stream=st.cuda_stream)
        a.push_messages_resident_dev(f["mask"], dm[k], verdict=verdicts[k], admit=admits[k], stream=st)
    st.synchronize()
    got = a.download_batch()
    # the yardstick: step by step through the host
    keep = []
    for k in range(3):
        r.solve_resident()
        tables, x = r.download_batch(), _solved(la, r)
        want = _statement(cfg, f["mask"], tables.counts, x.poses, cycles[k])
        keep.append(_slide_with_rows(r, name, want))
        torch.cuda.synchronize()
        assert verdicts[k].cpu().numpy().tolist() == want["verdict"].tolist(), (name, k)
        appended = want["verdict"] == M.APPENDED
        adm = admits[k].cpu().numpy()
        assert (adm[~appended] == 2).all() and (adm[appended] == 0).all(), (name, k, adm)
        assert appended.sum() > B // 2
    ref = r.download_batch()
    _same_batches(got, ref, f"{name} after three cycles")
    assert (got.counts[:, 0] == np.minimum(wb.counts[:, 0] + (np.stack([v.cpu().numpy() for v in verdicts]) == M.APPENDED).sum(axis=0), T)).all()
    if name == "uwb_only":
        assert got.p_info is not None   # the marginal carry made the table
    a.close(); r.close()


def test_one_turning_twist_step_within_the_bound(gpu):
    import torch
    import localization_amd as la
    name = "uwb_twist"
    f = FAMILIES[name]
    wb = _batch(la, name, seed=4)
    cfg = M.Config(T)
    msgs = _messages(name, 1, wb, seed=4, turning=True)
    a, r = _solver(la, wb), _solver(la, wb)
    for s in (a, r):
        s.upload(wb); _config(s, cfg); s.solve_resident()
    dm = _dev(M.masked(msgs, f["mask"]))
    torch.cuda.synchronize()
    a.push_messages_resident_dev(f["mask"], dm)
    got = a.download_batch()
    tables, x = r.download_batch(), _solved(la, r)
    want = _statement(cfg, f["mask"], tables.counts, x.poses, msgs)
    keep = _slide_with_rows(r, name, want)
    ref = r.download_batch()
    assert (want["ns"] == 1).sum() > B // 2
    worst = 0.0
    for b in range(B):
        ns = int(ref.counts[b, 3])
        if want["ns"][b] == 1:   # the appended row is the last one: its Z^-1 under the bound, everything else bitwise
            d = float(np.abs(got.s_val[b, ns - 1, :12] - ref.s_val[b, ns - 1, :12]).max())
            worst = max(worst, d)
            assert d <= M.TWIST_BOUND, (b, d)
            got.s_val[b, ns - 1, :12] = ref.s_val[b, ns - 1, :12]
    print(f"one turning TWIST step: largest |Z^-1 deviation| {worst:.3e} (bound {M.TWIST_BOUND:.3e})")
    _same_batches(got, ref, "turning twist")
    a.close(); r.close()
    del keep


# ---- 4. every verdict but APPENDED, beside appended neighbours ---------------------------------------------------------------------------------------------
def test_every_other_verdict_leaves_its_window_alone(gpu):
    import torch
    import localization_amd as la
    name = "uwb_twist"   # (its verdict admits every legal kind: two priors per pose, an EdgeSE3 per pair)
    cs = [c for c in M.causes(T) if c[0] != "nv_negative"]   # (a negative count cannot be uploaded)
    cs.append(("rejected", M.RANGE, None, M.REJECTED))
    n = 2 * len(cs)
    nvs = np.full(n, 3)
    for i, c in enumerate(cs):
        nvs[2 * i] = {"nv_zero": 1, "nv_beyond_T": NV_MAX, "rejected": T}.get(c[0], 3)
    wb = _batch(la, name, nvs=nvs, seed=5)
    for i, c in enumerate(cs):
        if c[0] == "nv_zero":
            wb.counts[2 * i] = 0
    s = _solver(la, wb)
    s.upload(wb); _config(s, M.Config(T)); s.solve_resident()
    before, x = s.download_batch(), _solved(la, s)
    nv, newest = _newest(before.counts, x.poses)
    rng = np.random.default_rng(M.RANDOM_SEED + 9)
    msgs = M.empty_messages(n)
    nv_dummy = nv.copy()
    for i, (cause, kind, change, verdict) in enumerate(cs):
        for b in (2 * i, 2 * i + 1):
            M.fill_message(rng, msgs, b, kind, newest[b], turning=False)
            msgs["distance"][b] = np.float32(M.estimate(newest[b], P.ANCH[msgs["anchor"][b]]) - 0.2)
        if cause == "rejected":
            msgs["distance"][2 * i] += np.float32(3.0)
        elif not cause.startswith("nv_"):
            change(msgs, nv_dummy, 2 * i)
    want = _statement(M.Config(T), ALL, before.counts, x.poses, msgs)
    assert want["verdict"].tolist() == [v for c in cs for v in (c[3], M.APPENDED)], list(zip([c[0] for c in cs], want["verdict"][::2]))
    dm = _dev(msgs)
    verdict, status, admit = (torch.full((n,), M.POISON_I, dtype=torch.int32, device="cuda") for _ in range(3))
    torch.cuda.synchronize()
    s.push_messages_resident_dev(ALL, dm, verdict=verdict, status=status, admit=admit)
    after, x_after = s.download_batch(), _solved(la, s)
    assert verdict.cpu().numpy().tolist() == want["verdict"].tolist()
    # (a window without poses is refused by the slide's first rule, every other one by its counts of -1)
    assert admit.cpu().numpy().tolist() == [c for cause in cs for c in (1 if cause[0] == "nv_zero" else 2, 0)] and status.cpu().numpy().tolist() == [c for _ in cs for c in (LOC_ERR_INVALID, 0)]
    refused = tuple(range(0, n, 2))
    for b in refused:   # every row of every table (used or not), the solved poses and the next solve's input estimates
        for t in P.TABLES:
            assert getattr(after, t)[b].tobytes() == getattr(before, t)[b].tobytes(), (cs[b // 2][0], t)
        assert x_after.poses[b].tobytes() == x.poses[b].tobytes(), cs[b // 2][0]
    rows = (want["pose"], (want["nr"], want["r_idx"].reshape(n, 2, 2), want["r_val"].reshape(n, 2, 5)), (want["np"], want["p_val"].reshape(n, 2, 18)),
            (want["ns"], want["s_idx"].reshape(n, 1, 4), want["s_val"].reshape(n, 1, 48)), want["drop"])
    start = before.copy(); start.poses[:] = x.poses
    slid = P.slide_plain_ref(la, start, *rows, refused=refused)
    P.assert_same_tables(after, slid, "neighbours", [b for b in range(n) if b not in refused])
    # TWIST with s == 0 needs trajectory_length 1: one-pose windows at their lag (build only)
    s.close()
    wb1 = _batch(la, name, nvs=np.ones(6, dtype=int), seed=6)
    s1 = _solver(la, wb1)
    s1.upload(wb1); _config(s1, M.Config(1)); s1.solve_resident()
    m1 = M.empty_messages(6)
    x1 = _solved(la, s1)
    for b in range(6):
        M.fill_message(rng, m1, b, M.TWIST if b % 2 else M.RANGE, x1.poses[b, 0])
        m1["distance"][b] = np.float32(M.estimate(x1.poses[b, 0], P.ANCH[m1["anchor"][b]]) + 0.1)
    got = _build(s1, ALL, m1)
    want1 = _statement(M.Config(1), ALL, wb1.counts, x1.poses, m1)
    M.assert_same_records(got, want1, m1, "T = 1")
    assert want1["verdict"].tolist() == [M.APPENDED, M.INVALID] * 3 and want1["nr"][0] == 1
    s1.close()


# ---- 5. host refusals ---------------------------------------------------------------------------------------------------------------------------------------
def test_host_refusals_launch_nothing(gpu):
    import torch
    import localization_amd as la
    name = "uwb_imu"
    mask = FAMILIES[name]["mask"]
    wb = _batch(la, name, nvs=(np.arange(12) % T) + 1, seed=8)
    msgs = _messages(name, 0, wb, seed=8)
    s = _solver(la, wb)
    s.upload(wb)
    dm, out = _dev(M.masked(msgs, mask)), _outputs(wb.B)
    torch.cuda.synchronize()

    def refused(call):
        with pytest.raises(la.LocalizationAmdError) as e:
            call()
        assert e.value.code == LOC_ERR_INVALID, e.value
        torch.cuda.synchronize()
        for k, v in out.items():
            assert (v.cpu().numpy() == (M.POISON_I if v.dtype == torch.int32 else M.POISON_D)).all(), k

    s.solve_resident()
    before, x = s.download_batch(), _solved(la, s)
    refused(lambda: s.message_rows_dev(mask, dm, out))                                    # no configuration
    refused(lambda: s.push_messages_resident_dev(mask, dm, verdict=out["verdict"]))
    refused(lambda: s.set_message_config(NV_MAX + 1))                                     # trajectory_length > nv_max
    refused(lambda: s.set_message_config(0))
    refused(lambda: s.message_rows_dev(mask, dm, out))                                    # ... and that left no configuration behind
    _config(s, M.Config(T))
    refused(lambda: s.message_rows_dev(mask, {k: v for k, v in dm.items() if k != "imu"}, out))      # NULL arrays under a mask bit
    refused(lambda: s.message_rows_dev(mask, {k: v for k, v in dm.items() if k != "distance"}, out))
    refused(lambda: s.message_rows_dev(mask, {k: v for k, v in dm.items() if k != "dt"}, out))
    refused(lambda: s.push_messages_resident_dev(mask, {k: v for k, v in dm.items() if k != "imu"}, verdict=out["verdict"]))
    refused(lambda: s.message_rows_dev(mask | 16, dm, out))                               # unknown bits
    refused(lambda: s.message_rows_dev(mask, dm, {k: v for k, v in out.items() if k != "new_s_val"}))   # a NULL output other than verdict
    after, x_after = s.download_batch(), _solved(la, s)
    for t in P.TABLES:
        assert getattr(after, t).tobytes() == getattr(before, t).tobytes(), t
    assert x_after.poses.tobytes() == x.poses.tobytes()
    s.upload(wb)                                                                          # no solve since the upload
    refused(lambda: s.message_rows_dev(mask, dm, out))
    refused(lambda: s.push_messages_resident_dev(mask, dm, verdict=out["verdict"]))
    s.solve_resident()
    s.message_rows_dev(mask, dm, {k: v for k, v in out.items() if k != "verdict"})        # verdict may be NULL
    torch.cuda.synchronize()
    assert (out["verdict"].cpu().numpy() == M.POISON_I).all() and (out["new_r_counts"].cpu().numpy() != M.POISON_I).all()
    s.close()


# ---- 6. position independence -------------------------------------------------------------------------------------------------------------------------------
def test_permuted_windows_give_permuted_outputs(gpu):
    import localization_amd as la
    name = "uwb_twist"
    s, wb, poses, _ = _family(name)
    perm = np.random.default_rng(M.RANDOM_SEED + 11).permutation(B)
    rng = np.random.default_rng(M.RANDOM_SEED + 12)
    nv, x = _newest(wb.counts, poses)
    msgs = M.empty_messages(B)
    for b in range(B):
        M.fill_message(rng, msgs, b, int(rng.choice(M.LEGAL_KINDS)), x[b])
    got = _build(s, ALL, msgs)
    wbp = wb.take(perm)
    sp = _solver(la, wbp)
    sp.upload(wbp); _config(sp, M.Config(T)); sp.solve_resident()
    used = np.arange(NV_MAX)[None, :] < wbp.counts[:, :1]
    assert _solved(la, sp).poses[used].tobytes() == poses[perm][used].tobytes()   # (the solve kernels do not depend on a window's position either)
    gotp = _build(sp, ALL, {k: v[perm] for k, v in msgs.items()})
    for f in M.FIELDS:
        assert gotp[f].tobytes() == got[f][perm].tobytes(), f
    sp.close()


# ---- 7. the pushed batch serves every resident call ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["uwb_imu", "uwb_twist"])
def test_after_a_push_the_resident_calls_match_a_fresh_upload(gpu, name):
    import torch
    import localization_amd as la
    f = FAMILIES[name]
    wb = _batch(la, name, seed=13)
    msgs = _messages(name, 0, wb, seed=13)
    s = _solver(la, wb)
    s.upload(wb); _config(s, M.Config(T)); s.solve_resident()
    dm = _dev(M.masked(msgs, f["mask"]))
    torch.cuda.synchronize()
    s.push_messages_resident_dev(f["mask"], dm)
    pushed = s.download_batch()
    assert (pushed.counts[:, 0] == np.minimum(wb.counts[:, 0] + 1, T)).sum() > B // 2
    fresh = _solver(la, pushed)
    fresh.upload(pushed)
    d = torch.device("cuda", 0)
    res = []
    for h in (s, fresh):
        h.solve_resident()
        cov = torch.zeros((B, NV_MAX, 36), dtype=torch.float64, device=d)
        mask, status = torch.zeros((B, NV_MAX), dtype=torch.int32, device=d), torch.zeros(B, dtype=torch.int32, device=d)
        h.covariance_resident(cov, mask, status)
        chi = [torch.zeros((B, max(c, 1)), dtype=torch.float64, device=d) for c in h.caps[1:]]
        total, active = torch.zeros(B, dtype=torch.float64, device=d), torch.zeros(B, dtype=torch.int32, device=d)
        h.edge_chi2_resident(*chi, total, active)
        solved = _solved(la, h)
        torch.cuda.synchronize()
        res.append((h.last_kernel_kind(), solved.poses.copy(), solved.result.copy(), [t.cpu().numpy() for t in (cov, mask, status, *chi, total, active)]))
    assert res[0][0] == res[1][0] and res[0][0] in KERNELS[name], (res[0][0], res[1][0])
    used = np.arange(NV_MAX)[None, :] < pushed.counts[:, :1]
    assert res[0][1][used].tobytes() == res[1][1][used].tobytes() and res[0][2].tobytes() == res[1][2].tobytes()
    for x, y in zip(res[0][3], res[1][3]):
        assert x.tobytes() == y.tobytes()
    s.close(); fresh.close()
