"""Publish and path records of a resident batch on the device (loc_window_publish_resident, loc_window_path_resident;
window_publish_kernel.hip; DESIGN.md §2, "Publish and path records of a resident batch").  The yardstick is the statement written from the
reference's behaviour (tests/_publish_ref.py) applied to download()'s poses and result and the resident counts, BIT FOR BIT on every output
array: every output is poisoned first and is three windows longer than the batch, so "left as the caller had it" is part of every comparison.

Smallest shapes: 130 windows (two full waves and a tail of two lanes), nv_max = trajectory_length = 12, four anchors.  The full-window
families are built and solved once and shared (_family); torch copies on ITS stream and the handle's stream does not wait for it: every test
synchronises before it hands pointers over."""
import ctypes as C
import functools

import numpy as np
import pytest

import _message_rows_ref as M
import _publish_ref as R
import _slide_plain_ref as P

pytestmark = pytest.mark.gpu

B, T = 130, 12
EXTRA = 3   # windows the output tensors are longer than the batch
LOC_ERR_INVALID = -1
INF = float("inf")
# family -> priors per pose, EdgeSE3 per pair, translation-only, the kinds of three consecutive cycles, kinds_mask, the resident solve's kernel
FAMILIES = {
    "uwb_only": dict(priors=1, se3=0, chain3=True, kinds=(M.RANGE,) * 3, mask=M.RANGE, kernels=("wave3_lm_kernel", "chain3_lm_kernel")),
    "uwb_imu": dict(priors=1, se3=0, chain3=False, kinds=(M.RANGE | M.IMU,) * 3, mask=M.RANGE | M.IMU, kernels=("wave6_lm_kernel",)),
    "uwb_twist": dict(priors=2, se3=1, chain3=False, kinds=(M.RANGE, M.TWIST, M.RANGE), mask=M.RANGE | M.TWIST, kernels=("wave6_lm_kernel<SE3>",)),
}
RAGGED = (np.arange(B) % T) + 1   # every count 1 .. T


def _batch(la, name, nvs=None, seed=0):
    """the family's windows: window i has nvs[i] poses (default: all full)"""
    f = FAMILIES[name]
    nvs = np.full(B, T) if nvs is None else np.asarray(nvs)
    streams = [P.Stream(8100 + 1000 * seed + i, T + 1, 1, f["priors"], f["se3"]) for i in range(len(nvs))]
    wb = P.window_batch(la, streams, nvs, P.caps_of(T, 1, f["priors"], f["se3"]))
    if f["chain3"]:   # nothing that turns a pose: identity rotations, no lever arm, translation information only
        wb.poses[:, :, :9] = np.eye(3).reshape(9)
        wb.r_val[:, :, 2:] = 0.0
        wb.p_val[:, :, :9] = np.eye(3).reshape(9); wb.p_val[:, :, 15:] = 0.0; wb.p_val[:, :, 12:15] = 4.0
    return wb


def _solver(la, wb, **kw):
    s = la.WindowSolver(P.ANCH, wb.B, *wb.caps, jacobian="analytic", **kw)
    s.set_option("resident_slide", 1)
    return s


def _state(la, s):
    """(counts, solved poses, result) of the resident batch, through the host"""
    wb = la.WindowBatch(s._resident, *s.caps)
    s.download(wb)
    return s.download_batch().counts.copy(), wb.poses.copy(), wb.result.copy()


@functools.lru_cache(maxsize=None)
def _family(name, ragged=False):
    """(solver, counts, solved poses, result, kernel): uploaded and solved once"""
    import localization_amd as la
    wb = _batch(la, name, RAGGED if ragged else None)
    s = _solver(la, wb)
    s.upload(wb); s.solve_resident()
    kind = s.last_kernel_kind()
    return (s,) + _state(la, s) + (kind,)


def _poison_d(*shape):
    return np.full(shape, R.POISON_D)


def _poison_i(*shape):
    return np.full(shape, R.POISON_I, dtype=np.int32)


def _dev(x):
    import torch
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(torch.device("cuda", 0))


def _publish_outputs(n):
    h = dict(flags=_poison_i(n + EXTRA), realtime=_poison_d(n + EXTRA, 7), optimized=_poison_d(n + EXTRA, 7), chi2=_poison_d(n + EXTRA),
             n_published=_poison_i(1))
    return h, {k: _dev(v) for k, v in h.items()}


def _host(d):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in d.items()}


def _publish(s, thr, tl=T, stream=None):
    """one publish call into poisoned outputs: (the poisoned host arrays, the device outputs on the host)"""
    import torch
    h, d = _publish_outputs(s._resident)
    torch.cuda.synchronize()
    s.publish_resident(thr, tl, d["flags"], d["realtime"], d["optimized"], d["chi2"], d["n_published"], stream=stream)
    return h, _host(d)


def _assert_publish(got, poisoned, counts, poses, result, thr, tl=T, what=""):
    flags, rt, opt, chi2, n = R.publish(counts, poses, result, thr, tl, poisoned["flags"], poisoned["realtime"], poisoned["optimized"], poisoned["chi2"])
    for name, want in (("flags", flags), ("realtime", rt), ("optimized", opt), ("chi2", chi2)):
        if not R.same_bits(got[name], want):
            bad = [b for b in range(len(want)) if got[name][b].tobytes() != want[b].tobytes()]
            raise AssertionError((what, name, bad[:8], got[name][bad[0]], want[bad[0]]))
    assert got["n_published"].tolist() == [n], (what, got["n_published"], n)
    return flags, n


def _path(s, first, count, tl=T, stream=None):
    import torch
    n = s._resident
    h = dict(path=_poison_d(n + EXTRA, count, 7), present=_poison_i(n + EXTRA, count))
    d = {k: _dev(v) for k, v in h.items()}
    torch.cuda.synchronize()
    s.path_resident(tl, d["path"], d["present"], first=first, count=count, stream=stream)
    return h, _host(d)


def _assert_path(got, poisoned, counts, poses, first, count, tl=T, what=""):
    n = len(counts)
    rows, present = R.path(counts, poses, tl, first, count, poisoned["path"][:n], poisoned["present"][:n])
    assert R.same_bits(got["present"][:n], present), (what, "present")
    assert R.same_bits(got["path"][:n], rows), (what, "path", np.argwhere(got["path"][:n].view(np.uint64) != rows.view(np.uint64))[:4])
    assert R.same_bits(got["present"][n:], poisoned["present"][n:]) and R.same_bits(got["path"][n:], poisoned["path"][n:]), (what, "beyond n")
    return rows, present


def _median_threshold(result):
    """a threshold from the batch's own solved chi2, with the split it must give: at least 20 and at most 110 of the 130 windows pass (for a
    batch of another size: some pass, some do not)"""
    chi = result[:, 0]
    thr = float(np.median(chi[np.isfinite(chi)]))
    below = int((chi < thr).sum())
    assert (20 <= below <= 110) if len(chi) == B else (0 < below < len(chi)), (below, thr)
    return thr


# ---- 1. the three resident chain shapes, full windows -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FAMILIES))
def test_full_windows_bit_for_bit(gpu, name):
    s, counts, poses, result, kind = _family(name)
    assert kind in FAMILIES[name]["kernels"], kind
    assert (counts[:, 0] == T).all()
    thr = _median_threshold(result)
    h, got = _publish(s, thr)
    flags, n = _assert_publish(got, h, counts, poses, result, thr, what=name)
    assert 20 <= n <= 110 and (flags[:B] & 2).all()
    assert s.last_kernel_kind() == kind
    assert s.last_covariance_ms() > 0.0
    # the optional outputs left out: the others are the same
    import torch
    h2, d2 = _publish_outputs(B)
    torch.cuda.synchronize()
    s.publish_resident(thr, T, d2["flags"], realtime=d2["realtime"])
    g2 = _host(d2)
    assert R.same_bits(g2["flags"], got["flags"]) and R.same_bits(g2["realtime"], got["realtime"])
    for k in ("optimized", "chi2", "n_published"):
        assert R.same_bits(g2[k], h2[k]), k
    for r in got["realtime"][:B][flags[:B] & 1 == 1]:
        assert abs(np.linalg.norm(r[3:]) - 1.0) < 1e-9 and r[6] >= 0


# ---- 2. the gate's edges ------------------------------------------------------------------------------------------------------------------------
class _DeviceDoubles:
    """a device array of doubles at a raw pointer, for torch.as_tensor"""

    def __init__(self, ptr, shape):
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr="<f8", data=(int(ptr), False), version=2)


def test_gate_edges(gpu):
    import torch
    import localization_amd as la
    wb = _batch(la, "uwb_only", seed=1)
    s = _solver(la, wb)
    s.upload(wb); s.solve_resident()
    _, _, res0 = _state(la, s)
    order = np.argsort(res0[:, 0])
    b_nan, b_small, b_edge = int(order[5]), int(order[20]), int(order[70])
    assert res0[b_small, 0] < res0[b_edge, 0]
    dres = torch.as_tensor(_DeviceDoubles(s.L.loc_window_result_device(s.h), (B, 8)), device=torch.device("cuda", 0))
    dres[b_nan, 0] = float("nan")
    torch.cuda.synchronize()
    counts, poses, result = _state(la, s)
    assert np.isnan(result[b_nan, 0]) and np.isfinite(np.delete(result[:, 0], b_nan)).all()
    edge = float(result[b_edge, 0])
    for thr, what in ((edge, "at"), (float(np.nextafter(edge, INF)), "above"), (INF, "inf"), (0.0, "zero")):
        h, got = _publish(s, thr)
        flags, n = _assert_publish(got, h, counts, poses, result, thr, what=what)
        assert not flags[b_nan] & 1, what
        if what == "at":
            assert not flags[b_edge] & 1 and flags[b_small] & 1
        if what == "above":
            assert flags[b_edge] & 1
        if what == "inf":
            assert n == B - 1 and (np.delete(flags[:B], b_nan) & 1).all()
        if what == "zero":
            assert n == 0 and not (flags[:B] & 1).any()
        assert np.isnan(got["chi2"][b_nan])
    s.close()


# ---- 3. ragged windows ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["uwb_only", "uwb_imu"])
def test_ragged_windows_and_paths(gpu, name):
    s, counts, poses, result, kind = _family(name, ragged=True)
    nv = counts[:, 0].astype(int)
    assert sorted(set(nv.tolist())) == list(range(1, T + 1))
    h, all_pub = _publish(s, INF)
    flags, n = _assert_publish(all_pub, h, counts, poses, result, INF, what=name)
    assert n == B
    assert ((flags[:B] & 2) != 0).tolist() == (T // 2 - (T - nv) >= 0).tolist()
    for b in np.flatnonzero(flags[:B] & 2):
        assert all_pub["optimized"][b].tobytes() == R.pose_record(poses[b, T // 2 - (T - nv[b])]).tobytes()
    # vertices2path, the destructor's tail, the newest pose alone
    for first, count in ((0, T), (T // 2, T - T // 2), (T - 1, 1), (3, 4)):
        hp, got = _path(s, first, count)
        rows, present = _assert_path(got, hp, counts, poses, first, count, what=(name, first, count))
        assert present.sum() == sum(max(0, min(first + count, T) - max(first, T - v)) for v in nv)
    hp, newest = _path(s, T - 1, 1)
    assert (newest["present"][:B] == 1).all() and R.same_bits(newest["path"][:B, 0], all_pub["realtime"][:B])
    hp, tail = _path(s, T // 2, T - T // 2)
    hp, full = _path(s, 0, T)
    assert R.same_bits(tail["path"][:B], full["path"][:B, T // 2:]) and R.same_bits(tail["present"][:B], full["present"][:B, T // 2:])
    assert s.last_kernel_kind() == kind


# ---- 4. untouched means untouched -----------------------------------------------------------------------------------------------------------------
def test_untouched_rows_keep_the_poison(gpu):
    s, counts, poses, result, _ = _family("uwb_imu", ragged=True)
    nv = counts[:, 0].astype(int)
    thr = _median_threshold(result)
    h, got = _publish(s, thr)
    flags, _ = _assert_publish(got, h, counts, poses, result, thr)
    poison7 = _poison_d(7).tobytes()
    unpublished = np.flatnonzero((flags[:B] & 1) == 0)
    no_opt = np.flatnonzero((flags[:B] & 3) == 1)
    assert len(unpublished) >= 20 and len(no_opt) >= 5
    for b in unpublished:
        assert got["realtime"][b].tobytes() == poison7 and got["optimized"][b].tobytes() == poison7
    for b in no_opt:
        assert got["realtime"][b].tobytes() != poison7 and got["optimized"][b].tobytes() == poison7
    for k in ("flags", "realtime", "optimized", "chi2"):
        assert R.same_bits(got[k][B:], h[k][B:]), k
    assert not np.isnan(got["chi2"][:B]).any()   # always written
    hp, path = _path(s, 0, T)
    absent = path["present"][:B] == 0
    assert absent.sum() == int((T - nv).sum()) > 0
    assert all(r.tobytes() == poison7 for r in path["path"][:B][absent])
    assert R.same_bits(path["path"][B:], hp["path"][B:]) and R.same_bits(path["present"][B:], hp["present"][B:])


# ---- 5. position independence ------------------------------------------------------------------------------------------------------------------------
def test_permuted_windows_give_permuted_outputs(gpu):
    import localization_amd as la
    s, counts, poses, result, _ = _family("uwb_imu", ragged=True)
    thr = _median_threshold(result)
    _, a = _publish(s, thr)
    _, pa = _path(s, 0, T)
    perm = np.random.default_rng(5).permutation(B)
    wb = _batch(la, "uwb_imu", RAGGED)
    pw = la.WindowBatch(B, *wb.caps)
    for name in P.TABLES:
        getattr(pw, name)[:] = getattr(wb, name)[perm]
    s2 = _solver(la, pw)
    s2.upload(pw); s2.solve_resident()
    c2, x2, r2 = _state(la, s2)
    assert R.same_bits(x2, poses[perm]) and R.same_bits(r2[:, 0], result[perm, 0])   # (the solve's own position independence)
    h, b = _publish(s2, thr)
    _assert_publish(b, h, c2, x2, r2, thr)
    _, pb = _path(s2, 0, T)
    for k in ("flags", "realtime", "optimized", "chi2"):
        assert R.same_bits(b[k][:B], a[k][:B][perm]), k
    assert b["n_published"].tolist() == a["n_published"].tolist()
    assert R.same_bits(pb["path"][:B], pa["path"][:B][perm]) and R.same_bits(pb["present"][:B], pa["present"][:B][perm])
    s2.close()


# ---- 6. in the loop ------------------------------------------------------------------------------------------------------------------------------------
def _messages(name, cycle, wb, seed):
    f = FAMILIES[name]
    rng = np.random.default_rng(M.RANDOM_SEED + 100 * seed + cycle)
    msgs = M.empty_messages(wb.B)
    for b in range(wb.B):
        nv = max(int(wb.counts[b, 0]), 1)
        M.fill_message(rng, msgs, b, f["kinds"][cycle], wb.poses[b, nv - 1], turning=False)
        if f["chain3"]:
            msgs["antenna"][b] = 0
        if b % 11 == 3:
            msgs["kind"][b] = 0
    return msgs


@pytest.mark.parametrize("name", list(FAMILIES))
def test_three_queued_cycles(gpu, name):
    import torch
    import localization_amd as la
    f = FAMILIES[name]
    wb = _batch(la, name, RAGGED, seed=3)
    cfg = M.Config(T)
    cycles = [{k: _dev(v) for k, v in M.masked(_messages(name, k, wb, 3), f["mask"]).items()} for k in range(3)]
    a, r = _solver(la, wb), _solver(la, wb)
    for s in (a, r):
        s.upload(wb)
        s.set_message_config(cfg.T, cfg.vmax, cfg.outlier, cfg.antenna)
    # the yardstick: a synchronisation and a download after every solve, the records formed on the host
    torch.cuda.synchronize()
    r.solve_resident()
    want = []
    for k in range(3):
        r.push_messages_resident_dev(f["mask"], cycles[k])
        r.solve_resident()
        torch.cuda.synchronize()
        counts, poses, result = _state(la, r)
        thr = _median_threshold(result)
        h = _publish_outputs(B)[0]
        want.append((thr, R.publish(counts, poses, result, thr, T, h["flags"], h["realtime"], h["optimized"], h["chi2"])))
    ref = r.download_batch()
    # the handle under test: everything queued on one stream, each cycle into its own outputs, ONE synchronisation at the end
    outs = [_publish_outputs(B)[1] for _ in range(3)]
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    a.solve_resident(stream=st.cuda_stream)
    for k in range(3):
        a.push_messages_resident_dev(f["mask"], cycles[k], stream=st)
        a.solve_resident(stream=st.cuda_stream)
        o = outs[k]
        a.publish_resident(want[k][0], T, o["flags"], o["realtime"], o["optimized"], o["chi2"], o["n_published"], stream=st)
    st.synchronize()
    for k in range(3):
        got = _host(outs[k])
        flags, rt, opt, chi2, n = want[k][1]
        for key, w in (("flags", flags), ("realtime", rt), ("optimized", opt), ("chi2", chi2)):
            assert R.same_bits(got[key], w), (name, k, key)
        assert got["n_published"].tolist() == [n] and 20 <= n <= 110, (name, k, n)
    got = a.download_batch()
    P.assert_same_tables(got, ref, f"{name} after three cycles")   # the publish calls write nothing of the batch
    assert (got.p_info is None) == (ref.p_info is None)
    if got.p_info is not None:
        for w in range(B):
            m = int(got.counts[w, 2])
            assert got.p_info[w, :m].tobytes() == ref.p_info[w, :m].tobytes(), (name, "p_info", w)
    assert (got.counts[:, 0] > wb.counts[:, 0]).sum() > B // 2   # the windows did grow
    a.close(); r.close()


# ---- 7. other structures -------------------------------------------------------------------------------------------------------------------------------
def _check_everything(la, s, tl, what):
    kind = s.last_kernel_kind()
    counts, poses, result = _state(la, s)
    thr = _median_threshold(result)
    for t in (thr, INF):
        h, got = _publish(s, t, tl)
        _assert_publish(got, h, counts, poses, result, t, tl, what=what)
    for first, count in ((0, tl), (tl // 2, tl - tl // 2), (tl - 1, 1)):
        hp, got = _path(s, first, count, tl)
        _assert_path(got, hp, counts, poses, first, count, tl, what=(what, first, count))
    assert s.last_kernel_kind() == kind
    return kind, counts


def test_forest_and_general_batches(gpu):
    import localization_amd as la
    from test_gpu_tree_parity import ANCH, _forest_batch
    wb = _forest_batch(la, np.random.default_rng(8300), 256, 24, 4, True)   # two key-frame trees per window
    s = la.WindowSolver(ANCH, wb.B, *wb.caps, jacobian="analytic", bw_max=23)
    s.upload(wb); s.solve_resident()
    kind, _ = _check_everything(la, s, 24, "forest")
    assert kind in ("tree_wave_kernel", "tree_lm_kernel"), kind
    s.close()
    wb, _, _ = P.case_batch(la, "ragged")   # 1, 2, 4 and 6 poses under nv_max = 9
    s = _solver(la, wb, chain_threshold=0)   # (threshold 0: never anything but the general kernel)
    s.upload(wb); s.solve_resident()
    for tl in (9, 6):
        kind, counts = _check_everything(la, s, tl, f"general T={tl}")
    assert kind == "window_lm_kernel" and sorted(set(counts[:, 0].tolist())) == [1, 2, 4, 6]
    s.close()


# ---- 8. refusals launch nothing ---------------------------------------------------------------------------------------------------------------------------
def _refused(call, word):
    import localization_amd as la
    from localization_amd._lib import LocalizationAmdError
    with pytest.raises(LocalizationAmdError) as e:
        call()
    assert e.value.code == LOC_ERR_INVALID and word in str(e.value), (word, str(e.value))


def test_refusals_launch_nothing(gpu):
    import torch
    import localization_amd as la
    wb = _batch(la, "uwb_imu", seed=2)
    s = _solver(la, wb)
    h, d = _publish_outputs(B)
    hp = dict(path=_poison_d(B, T, 7), present=_poison_i(B, T))
    dp = {k: _dev(v) for k, v in hp.items()}
    torch.cuda.synchronize()
    pub = lambda thr=INF, tl=T, flags=d["flags"]: s.publish_resident(thr, tl, flags, d["realtime"], d["optimized"], d["chi2"], d["n_published"])
    path = lambda tl=T, first=0, count=T, p=dp["path"], q=dp["present"]: s.path_resident(tl, p, q, first=first, count=count)
    vp = lambda t: C.c_void_p(t.data_ptr())
    L = s.L
    assert L.loc_window_publish_resident(None, None, 1.0, T, vp(d["flags"]), None, None, None, None) == LOC_ERR_INVALID
    assert b"nothing uploaded" in L.loc_last_error()
    assert L.loc_window_path_resident(None, None, T, 0, T, vp(dp["path"]), vp(dp["present"])) == LOC_ERR_INVALID
    assert b"nothing uploaded" in L.loc_last_error()
    _refused(pub, "nothing uploaded"); _refused(path, "nothing uploaded")
    s.upload(wb)
    _refused(pub, "no resident solve"); _refused(path, "no resident solve")
    s.solve_resident()
    for tl in (0, -3, T + 1):
        _refused(lambda: pub(tl=tl), "trajectory_length"); _refused(lambda: path(tl=tl, count=1), "trajectory_length")
    _refused(lambda: pub(thr=float("nan")), "NaN")
    _refused(lambda: pub(flags=None), "flags_dev")
    _refused(lambda: path(first=-1), "first"); _refused(lambda: path(count=0), "count"); _refused(lambda: path(first=1, count=T), "first + count")
    _refused(lambda: path(tl=T - 1, first=0, count=T), "first + count")
    _refused(lambda: path(p=None), "path_dev"); _refused(lambda: path(q=None), "present_dev")
    got, gotp = _host(d), _host(dp)
    for k in h:
        assert R.same_bits(got[k], h[k]), k
    for k in hp:
        assert R.same_bits(gotp[k], hp[k]), k
    # a following solve and publish work
    s.solve_resident()
    counts, poses, result = _state(la, s)
    h, got = _publish(s, INF)
    _, n = _assert_publish(got, h, counts, poses, result, INF)
    assert n == B
    # windows longer than trajectory_length: the caller's inconsistency — flags 0, every row untouched, chi2 still written
    h, got = _publish(s, INF, T - 1)
    flags, n = _assert_publish(got, h, counts, poses, result, INF, T - 1)
    assert n == 0 and not flags[:B].any()
    assert R.same_bits(got["realtime"], h["realtime"]) and R.same_bits(got["optimized"], h["optimized"])
    assert R.same_bits(got["chi2"][:B], result[:, 0])
    hq, gq = _path(s, 0, T - 1, T - 1)
    _assert_path(gq, hq, counts, poses, 0, T - 1, T - 1)
    assert not gq["present"][:B].any() and R.same_bits(gq["path"], hq["path"])
    s.close()
