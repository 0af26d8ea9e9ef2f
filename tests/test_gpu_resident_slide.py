"""The resident fixed-lag slide on the GPU (loc_window_slide_resident, loc_window_download_tables; DESIGN.md §2, "The resident slide"), held BIT
FOR BIT to the host composition the project already trusts:

    resident chain:  solve_resident -> slide_resident -> solve_resident -> ...
    host chain:      solve -> marginal_prior(., 0) -> tests/_slide_ref.slide_ref -> solve -> ...

No tolerance anywhere: a resident solve has the host solve's bits and a resident covariance the host covariance's (asserted elsewhere), the
marginal is marginal_prior_kernel itself, and the re-pack only moves rows.  Eight windows per case (tests/_slide_ref.CASES)."""
import ctypes as C

import numpy as np
import pytest

import _fixed_lag as F
import _slide_ref as S

pytestmark = pytest.mark.gpu

LOC_ERR_INVALID, LOC_ERR_UNSUPPORTED, LOC_ERR_SINGULAR = -1, -5, -6
STRUCTURED = "prior_information_structured"
KIND_AFTER = {1: "wave3_lm_kernel", 0: "window_lm_kernel"}   # with a table: the structured option keeps the wave kernel, without it the general one


def _solver(la, wb, jac="numeric", structured=1, slide=1):
    s = la.WindowSolver(F.ANCH, wb.B, *wb.caps, jacobian=jac)
    s.set_option(STRUCTURED, structured)
    if slide is not None:
        s.set_option("resident_slide", slide)
    return s


def _used(wb):
    return np.arange(wb.caps[0])[None, :] < wb.counts[:, :1]


def _outs(B, poison=None):
    import torch
    dev = torch.device("cuda", 0)
    out = (torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros((B, 48), dtype=torch.float64, device=dev),
           torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev))
    if poison is not None:
        for t in out:
            t.fill_(poison)
    torch.cuda.synchronize()   # (torch fills on ITS stream; the handle's stream does not wait for it: a caller orders its own writes)
    return out


def _fetch(out):
    import torch
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _same_solve(la, r, host, what):
    """the resident solve's poses, chi2s, lambda, iteration and trial counts against the host solve's"""
    got = la.WindowBatch(host.B, *host.caps)
    r.download(got)
    u = _used(host)
    assert got.poses[u].tobytes() == host.poses[u].tobytes(), (what, np.abs(got.poses[u] - host.poses[u]).max())
    assert got.result[:, :6].tobytes() == host.result[:, :6].tobytes(), (what, got.result[:, :6], host.result[:, :6])


def _chain(la, name, jac, structured, slides, drops=None, first=None, stream=None, order=None):
    """Both chains side by side, everything compared after every step; returns the host chain's batches and marginals.  drops: drop_oldest per
    slide (default: the case's); first: (batch, chains, spec) in the place of the case's; order: the windows' positions in the batch."""
    wb, chains, spec = S.case_batch(la, name) if first is None else first
    if order is not None:
        wb, chains = wb.take(order), [chains[k] for k in order]
        spec = dict(spec, consumed=spec["consumed"][order], drop=None if spec["drop"] is None else spec["drop"][order])
    r, h = _solver(la, wb, jac, structured), _solver(la, wb, jac, structured, slide=None)
    r.upload(wb)
    g = wb.copy()
    trail = []
    for step in range(slides + 1):
        what = f"{name} {jac} structured={structured} step {step}"
        r.solve_resident(None if stream is None else C.c_void_p(stream.cuda_stream))
        kind = r.last_kernel_kind()
        h.solve(g)
        _same_solve(la, r, g, what)
        h.upload(g); h.solve_resident()   # a fresh upload of the same tables takes the same kernel
        assert kind == h.last_kernel_kind(), (what, kind, h.last_kernel_kind())
        if step:
            assert kind == KIND_AFTER[structured], (what, kind)
        if step == slides:
            break
        if drops is not None:
            spec["drop"] = drops[step]
        pose, ranges, priors, drop = S.next_inputs(g, chains, spec)
        out = _outs(g.B)
        r.slide_resident(pose, ranges, priors, drop, out=out, stream=stream)
        for a in (pose, *ranges, *(priors or ())):   # the caller's arrays, overwritten right after the call: nothing reads them any more
            a[...] = -77
        pose2, ranges2, priors2, _ = _again(g, chains, spec)
        slot, prior, _, _, rank, status = h.marginal_prior(g, 0)
        dropped = np.ones(g.B, dtype=bool) if drop is None else drop != 0
        want = (np.where(dropped, slot, -1), np.where(dropped[:, None], prior, 0.0), np.where(dropped, rank, 0), np.where(dropped, status, 0))
        got = _fetch(out)
        for k, field in enumerate(("slot", "prior", "rank", "status")):
            assert got[k].tobytes() == want[k].astype(got[k].dtype).tobytes(), (what, field, got[k], want[k], got[0], got[2], got[3])
        g = S.slide_ref(la, g, slot, prior, pose2, ranges2, priors2, drop)
        S.assert_same_tables(r.download_batch(), g, what)
        trail.append((g.copy(), want))
    r.close(); h.close()
    return trail


def _again(g, chains, spec):
    """the inputs of the slide just made, built again (the first set was overwritten on purpose)"""
    back = dict(spec, consumed=spec["consumed"] - 1)
    return S.next_inputs(g, chains, back)


# ---- 1. bit for bit against the host composition ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("structured", [1, 0])
@pytest.mark.parametrize("jac", ["analytic", "numeric"])
def test_three_slides_of_a_window_of_six(gpu, jac, structured):
    import localization_amd as la
    trail = _chain(la, "plain", jac, structured, 3)
    for _, (slot, _, rank, status) in trail:
        assert (slot == 1).all() and (rank >= 1).all() and not status.any()


# ---- 2. the re-packed tables ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in S.CASES if n != "plain"])
def test_tables_after_each_slide(gpu, name):
    import localization_amd as la
    trail = _chain(la, name, "numeric", 1, 3)
    slot, prior, rank, status = trail[0][1]
    if name == "missing":
        assert (slot[0::2] == -1).all() and (slot[1::2] == 1).all() and (trail[0][0].counts[0::2, 2] == 0).all()
    if name == "one_range":   # the zero row IS inserted; the neighbours are ordinary rank >= 1 windows
        assert (status[[2, 5]] == LOC_ERR_SINGULAR).all() and not status[[0, 1, 3, 4, 6, 7]].any() and (slot == 1).all()
        assert (trail[0][0].counts[:, 2] == 1).all() and not trail[0][0].p_info[[2, 5], 0].any() and (rank[[0, 1, 3, 4, 6, 7]] >= 1).all()
    if name == "table":       # the even windows' caller-set matrix sat on slot 0 and went into the marginal; the odd windows' moved from slot 3 to 2
        assert not status.any() and (trail[0][0].counts[:, 2] == [1, 2] * 4).all() and (trail[0][0].p_idx[1::2, 1] == 2).all()
    if name == "ragged":      # the one-pose windows: dropped -> the new pose alone; grown -> two poses
        assert trail[0][0].counts[[0, 4], 0].tolist() == [1, 2] and slot[0] == -1
    if name == "long":
        assert (trail[0][0].counts[:, 1] == 99).all() and (trail[0][0].counts[:, 2] == 4).all()


# ---- 3. growing to the lag --------------------------------------------------------------------------------------------------------------------------
def test_growing_from_one_pose_to_the_lag(gpu):
    import localization_amd as la
    chains = [F.Chain(8400 + i, 9, 3 + i % 3) for i in range(8)]
    wb = la.WindowBatch(8, *S.caps_for(6))
    for i, ch in enumerate(chains):
        F.add_chain_poses(wb, i, ch, 0, 1)
    spec = dict(consumed=np.ones(8, dtype=int), drop=None)
    grow, slide = np.zeros(8, dtype=np.int32), np.ones(8, dtype=np.int32)
    trail = _chain(la, "grow", "numeric", 1, 7, drops=[grow] * 5 + [slide] * 2, first=(wb, chains, spec))
    assert [int(t[0].counts[0, 0]) for t in trail] == [2, 3, 4, 5, 6, 6, 6]
    assert (trail[4][1][0] == -1).all() and (trail[5][1][0] == 1).all()


# ---- 4. consistency afterwards ------------------------------------------------------------------------------------------------------------------------
def test_covariances_after_a_slide_have_the_host_calls_bits(gpu):
    import torch
    import localization_amd as la
    wb, chains, spec = S.case_batch(la, "plain")
    r, h = _solver(la, wb), _solver(la, wb, slide=None)
    r.upload(wb); r.solve_resident()
    r.slide_resident(*S.next_inputs(wb, chains, spec))
    r.solve_resident()
    now = r.download_batch()
    r.download(now)   # the solved poses
    B, nvm = now.B, now.caps[0]
    pairs = np.array([[0, nvm - 1], [nvm - 1, 0], [2, 2], [1, 0]], dtype=np.int32)
    dev = torch.device("cuda", 0)
    tc = torch.zeros((B, nvm, 36), dtype=torch.float64, device=dev); tj = torch.zeros_like(tc)
    tm = torch.zeros((B, nvm), dtype=torch.int32, device=dev); ts = torch.zeros(B, dtype=torch.int32, device=dev)
    tx = torch.zeros((B, len(pairs), 36), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    r.covariance_resident(tc, tm, ts)
    r.joint_covariance_resident(pairs, None, tj, tm, ts, tx)
    torch.cuda.synchronize()
    cov, mask, status = h.covariance(now)
    jcov, _, _, cross = h.joint_covariance(now, pairs)
    assert not status.any() and np.isfinite(cov).all()
    assert tc.cpu().numpy().tobytes() == cov.reshape(B, nvm, 36).tobytes() and tj.cpu().numpy().tobytes() == jcov.reshape(B, nvm, 36).tobytes()
    assert tx.cpu().numpy().tobytes() == cross.reshape(B, len(pairs), 36).tobytes()
    assert tm.cpu().numpy().tobytes() == mask.tobytes() and not ts.cpu().numpy().any()
    r.close(); h.close()


def test_a_second_stream_and_another_position_give_the_same_bits(gpu):
    import torch
    import localization_amd as la
    base = _chain(la, "zprior", "numeric", 1, 2)
    other = _chain(la, "zprior", "numeric", 1, 2, stream=torch.cuda.Stream())
    order = np.array([6, 3, 0, 5, 2, 7, 4, 1])   # (parity kept: the case appends a prior in the odd windows)
    moved = _chain(la, "zprior", "numeric", 1, 2, order=order)
    for (a, ma), (b, mb), (c, mc) in zip(base, other, moved):
        S.assert_same_tables(b, a, "second stream")
        S.assert_same_tables(c, a.take(order), "another position")
        for x, y, z in zip(ma, mb, mc):
            assert x.tobytes() == y.tobytes() and x[order].tobytes() == z.tobytes()


def test_a_small_host_solve_between_two_slides_leaves_the_chain_alone(gpu):
    import localization_amd as la
    other = S.case_batch(la, "doubled")[0]
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    final = []
    for disturb in (False, True):
        wb, chains, spec = S.case_batch(la, "plain")
        s = _solver(la, wb)
        s.upload(wb); s.solve_resident()
        s.slide_resident(*S.next_inputs(wb, chains, spec))
        if disturb:   # (the C call itself: the wrapper's solve() would first hand the other batch's table, none, to the handle)
            o = other.copy()
            assert s.L.loc_window_solve_host(s.h, o.B, o.counts.ctypes.data_as(ip), o.poses.ctypes.data_as(dp), o.r_idx.ctypes.data_as(ip),
                                             o.r_val.ctypes.data_as(dp), o.p_idx.ctypes.data_as(ip), o.p_val.ctypes.data_as(dp),
                                             o.s_idx.ctypes.data_as(ip), o.s_val.ctypes.data_as(dp), o.result.ctypes.data_as(dp)) == 0
        s.solve_resident()
        s.slide_resident(*S.next_inputs(s.download_batch(), chains, spec))
        s.solve_resident()
        got = s.download_batch()
        s.download(got)
        final.append(got)
        s.close()
    S.assert_same_tables(final[1], final[0], "after a host solve of another batch")
    assert final[1].result[:, :6].tobytes() == final[0].result[:, :6].tobytes()


def _last_rows(ranges, keep):
    """the last `keep` new rows of every window (tests/_slide_ref.new_rows: the anchor ranges, then the smoothness edge) under nr_new_max = keep"""
    rc, ri, rv = ranges
    B = len(rc)
    counts = np.minimum(rc, keep).astype(np.int32)
    r_idx, r_val = np.zeros((B, keep, 2), dtype=np.int32), np.zeros((B, keep, 5))
    for b in range(B):
        r_idx[b, :counts[b]] = ri[b, rc[b] - counts[b]:rc[b]]; r_val[b, :counts[b]] = rv[b, rc[b] - counts[b]:rc[b]]
    return counts, r_idx, r_val


def test_growing_input_blocks_and_alternating_entries(gpu):
    """One handle, three windows of four poses: host slides with nr_new_max = 1, then 2 (the staged input block grows), a slide from device
    arrays (the mirror goes stale), a host slide with seven row slots (the mirror is fetched, the block grows again).  After every slide the
    tables are tests/_slide_ref.py's, bit for bit."""
    import torch
    import localization_amd as la
    chains = [F.Chain(8600 + i, 9, 3 + i % 3) for i in range(3)]
    wb = la.WindowBatch(3, *S.caps_for(4))
    for i, ch in enumerate(chains):
        F.add_chain_poses(wb, i, ch, 0, 4)
    r, h = _solver(la, wb), _solver(la, wb, slide=None)
    r.upload(wb)
    g = wb.copy()
    dev = torch.device("cuda", 0)
    for step, (keep, entry) in enumerate(((1, "host"), (2, "host"), (None, "device"), (None, "host"))):
        what = f"step {step}: {entry} entry, nr_new_max {keep or F.NA_MAX + 2}"
        r.solve_resident()
        h.solve(g)
        _same_solve(la, r, g, what)
        pose, ranges = S.new_rows(chains, np.full(3, 4 + step), np.full(3, 3))
        if keep is not None:
            ranges = _last_rows(ranges, keep)
        assert ranges[1].shape[1] == (keep or F.NA_MAX + 2)
        out = _outs(3)
        if entry == "host":
            r.slide_resident(pose, ranges, None, None, out=out)
        else:
            t_in = [torch.from_numpy(a.copy()).to(dev) for a in (pose, *ranges)]
            admit = torch.full((3,), -77, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            r.slide_resident_dev(t_in[0], tuple(t_in[1:]), None, None, out=(*out, admit))
            torch.cuda.synchronize()
            assert not admit.cpu().numpy().any()
        slot, prior, _, _, rank, status = h.marginal_prior(g, 0)
        got = _fetch(out)
        for k, want in enumerate((slot, prior, rank, status)):
            assert got[k].tobytes() == want.astype(got[k].dtype).tobytes(), (what, k, got[k], want)
        g = S.slide_ref(la, g, slot, prior, pose, ranges, None, None)
        S.assert_same_tables(r.download_batch(), g, what)
    r.solve_resident()
    h.solve(g)
    _same_solve(la, r, g, "after the last slide")
    r.close(); h.close()


# ---- 5. refusals leave the batch and the outputs alone -------------------------------------------------------------------------------------------------
def _refused(la, s, code, args, **kw):
    before = s.download_batch()
    out = _outs(before.B, poison=-77)
    with pytest.raises(la.LocalizationAmdError) as e:
        s.slide_resident(*args, out=out, **kw)
    assert e.value.code == code, (e.value, code)
    for t in _fetch(out):
        assert (t == -77).all()
    after = s.download_batch()
    for name in ("counts", "poses", "r_idx", "r_val", "p_idx", "p_val"):
        assert getattr(after, name).tobytes() == getattr(before, name).tobytes(), name
    assert (after.p_info is None) == (before.p_info is None) and (after.p_info is None or after.p_info.tobytes() == before.p_info.tobytes())


def _ready(la, name="plain", change=None, solve=True, slide=1, caps=None):
    wb, chains, spec = S.case_batch(la, name)
    if caps is not None:   # the same windows under a smaller nr_max
        small = la.WindowBatch(8, *caps)
        small.counts[:] = wb.counts; small.poses[:] = wb.poses; small.p_idx[:] = wb.p_idx; small.p_val[:] = wb.p_val
        small.r_idx[:] = wb.r_idx[:, :caps[1]]; small.r_val[:] = wb.r_val[:, :caps[1]]
        wb = small
    if change is not None:
        change(wb)
    s = _solver(la, wb, slide=slide)
    s.upload(wb)
    if solve:
        s.solve_resident()
    pose, ranges, priors, drop = S.next_inputs(wb, chains, spec)
    return s, wb, chains, spec, [pose, ranges, priors, drop]


def _rotation_entry(wb):
    wb.p_info = np.zeros((8, S.NP_MAX, 36)); wb.p_info[:, :, 3 * 6 + 3] = 40.0


def _lever_arm1(wb):
    wb.r_off1 = np.zeros((8, wb.caps[1], 3)); wb.r_off1[3, 0] = (0.1, 0, 0)


def _long_edge(wb):
    wb.add_range(2, 0, 2, 0.0, F.SMOOTH_INFO)


def _lever_arm0(wb):
    wb.r_val[1, 0, 2:5] = (0.05, 0, 0)


@pytest.mark.parametrize("how", ["option_0", "unsolved", "six_dof", "forest", "endpoint1", "rotation_table"])
def test_refused_batches(gpu, how):
    import localization_amd as la
    code = LOC_ERR_INVALID if how in ("option_0", "unsolved") else LOC_ERR_UNSUPPORTED
    change = {"six_dof": _lever_arm0, "forest": _long_edge, "endpoint1": _lever_arm1, "rotation_table": _rotation_entry}.get(how)
    s, _, _, _, args = _ready(la, change=change, solve=how != "unsolved", slide=0 if how == "option_0" else 1)
    if how == "unsolved":   # (nothing to download yet either: the refusal is all there is to see)
        with pytest.raises(la.LocalizationAmdError) as e:
            s.slide_resident(*args)
        assert e.value.code == code
    else:
        _refused(la, s, code, args)
    s.close()


@pytest.mark.parametrize("how", ["slot_nv_minus_3", "new_lever_arm", "nr_max", "np_max", "nv_max", "count"])
def test_refused_rows(gpu, how):
    import localization_amd as la
    code = LOC_ERR_UNSUPPORTED if how == "new_lever_arm" else LOC_ERR_INVALID
    if how == "nr_max":       # a doubled link in the fullest window under an nr_max that holds exactly what is there
        wb0 = S.case_batch(la, "plain")[0]
        full = int(np.argmax(wb0.counts[:, 1]))
        s, wb, chains, spec, args = _ready(la, caps=(6, int(wb0.counts[full, 1]), S.NP_MAX, 0))
        args[0], args[1] = S.new_rows(chains, spec["consumed"] - 1, np.full(8, 5), doubled=(full,))
    elif how == "np_max":     # three kept priors, the carried one and a new one
        s, wb, chains, spec, args = _ready(la, "long")
        pv = np.zeros((8, 1, 18)); pv[:, 0, 0] = pv[:, 0, 4] = pv[:, 0, 8] = 1.0; pv[:, 0, 12:] = S.Z_INFO
        args[2] = (np.ones(8, dtype=np.int32), pv)
    else:
        s, wb, chains, spec, args = _ready(la)
    pose, (rc, ri, rv), priors, drop = args
    if how == "slot_nv_minus_3":
        ri[6, int(rc[6]) - 1] = (5, 3)
    if how == "new_lever_arm":
        rv[4, 0, 4] = 0.02
    if how == "nv_max":       # a full window that only grows, its rows on slot 6
        args[3] = np.array([1, 1, 1, 0, 1, 1, 1, 1], dtype=np.int32)
        args[0], args[1] = S.new_rows(chains, spec["consumed"] - 1, 6 - args[3])
    if how == "count":
        rc[3] = ri.shape[1] + 1
    _refused(la, s, code, args)
    s.close()


# ---- 6. option 0 is the parent ------------------------------------------------------------------------------------------------------------------------
def test_without_the_option_nothing_moves(gpu):
    """a handle whose option was never touched: upload, resident solve and resident covariance have the host path's bits, as before"""
    import torch
    import localization_amd as la
    wb, _, _ = S.case_batch(la, "zprior")
    s = la.WindowSolver(F.ANCH, wb.B, *wb.caps, jacobian="numeric")
    host = wb.copy()
    s.solve(host)
    s.upload(wb); s.solve_resident()
    _same_solve(la, s, host, "option never touched")
    B, nvm = wb.B, wb.caps[0]
    dev = torch.device("cuda", 0)
    tc = torch.zeros((B, nvm, 36), dtype=torch.float64, device=dev)
    tm = torch.zeros((B, nvm), dtype=torch.int32, device=dev); ts = torch.zeros(B, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    s.covariance_resident(tc, tm, ts)
    torch.cuda.synchronize()
    cov, mask, status = s.covariance(host)
    assert tc.cpu().numpy().tobytes() == cov.reshape(B, nvm, 36).tobytes() and tm.cpu().numpy().tobytes() == mask.tobytes() and not status.any()
    s.close()
