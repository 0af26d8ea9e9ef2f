"""The resident slide from device arrays (loc_window_slide_resident_dev; DESIGN.md §2, "The resident slide"): the per-window inputs sit in
torch device tensors, each wave admits its own window, the host makes no pass over them.  The yardstick everywhere is the host entry point
loc_window_slide_resident on a second handle, BIT FOR BIT: both apply the same rule to the same inputs with the same two kernels' arithmetic, so
no tolerance is involved.  Eight windows per case (tests/_slide_ref.CASES); the refused windows are tests/_slide_dev_cases.py's, which
tests/test_resident_slide_dev_cpu.py holds to the host rule without a GPU.

torch copies the inputs on ITS stream and the handle's stream does not wait for it: every test synchronises before it hands pointers over."""
import ctypes as C
import types

import numpy as np
import pytest

import _fixed_lag as F
import _slide_dev_cases as K
import _slide_ref as S

pytestmark = pytest.mark.gpu

LOC_ERR_INVALID, LOC_ERR_UNSUPPORTED = -1, -5
STRUCTURED = "prior_information_structured"
POISON = -77
CHAIN3_SLIDE_TABLES = ("counts", "poses", "r_idx", "r_val", "p_idx", "p_val")   # the tables a chain3 slide touches: such windows have no EdgeSE3


def _solver(la, wb, jac="numeric", structured=1, slide=1, anchors=F.ANCH):
    s = la.WindowSolver(anchors, wb.B, *wb.caps, jacobian=jac)
    s.set_option(STRUCTURED, structured)
    s.set_option("resident_slide", slide)
    return s


def _plan(la, name, slides):
    """(batch, the inputs of `slides` consecutive slides of a case) — the counts evolve by the rule (nv + 1 - dropped), so that no test has to
    read them back between two slides"""
    wb, chains, spec = S.case_batch(la, name)
    counts = wb.counts.copy()
    steps = []
    for _ in range(slides):
        pose, ranges, priors, drop = S.next_inputs(types.SimpleNamespace(counts=counts), chains, spec)
        steps.append((pose, ranges, priors, drop))
        counts = counts.copy()
        counts[:, 0] += 1 - (1 if drop is None else (drop != 0).astype(np.int32))
    return wb, steps


def _dev(inputs):
    """(new_pose, new_ranges, new_priors, drop_oldest) as torch device tensors, in the order of slide_resident_dev's arguments"""
    import torch
    d = torch.device("cuda", 0)
    t = lambda a, dt: torch.from_numpy(np.array(a, dtype=dt)).to(d)   # (a copy: the inputs stay the caller's)
    pose, ranges, priors, drop = inputs
    B = len(pose)
    return (t(pose, np.float64),
            None if ranges is None else (t(ranges[0], np.int32), t(ranges[1], np.int32), t(ranges[2], np.float64)),
            None if priors is None else (t(priors[0], np.int32), t(priors[1], np.float64)),
            None if drop is None else t(np.broadcast_to(drop, (B,)), np.int32))


def _outs(B, n=5):
    """(slot, prior, rank, status[, admit]) poisoned"""
    import torch
    d = torch.device("cuda", 0)
    out = [torch.full((B,), POISON, dtype=torch.int32, device=d), torch.full((B, 48), float(POISON), dtype=torch.float64, device=d)]
    out += [torch.full((B,), POISON, dtype=torch.int32, device=d) for _ in range(n - 2)]
    return tuple(out)


def _fetch(out):
    import torch
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _solved(la, s):
    wb = la.WindowBatch(s._resident, *s.caps)
    s.download(wb)
    return wb


def _same_solve(la, a, b, what, windows=None):
    """two handles' last resident solves: optimised poses and results (chi2s, lambda, iteration and trial counts), byte for byte"""
    x, y = _solved(la, a), _solved(la, b)
    w = slice(None) if windows is None else list(windows)
    used = (np.arange(x.caps[0])[None, :] < a.download_batch().counts[:, :1])[w]   # (a solve leaves the slots beyond nv as they were)
    assert x.poses[w][used].tobytes() == y.poses[w][used].tobytes(), (what, np.abs(x.poses[w][used] - y.poses[w][used]).max())
    assert x.result[w, :6].tobytes() == y.result[w, :6].tobytes(), (what, x.result[w, :6], y.result[w, :6])
    assert a.last_kernel_kind() == b.last_kernel_kind(), (what, a.last_kernel_kind(), b.last_kernel_kind())


def _same_outputs(got, want, what, windows=None):
    w = slice(None) if windows is None else list(windows)
    for k, field in enumerate(("slot", "prior", "rank", "status")):
        assert got[k][w].tobytes() == want[k][w].tobytes(), (what, field, got[k], want[k])


def _pair_of_chains(la, name, jac, structured, slides, stream=None, order=None):
    """`slides` cycles of (solve, slide) through the device entry on one handle and through the host entry on another, compared after every
    step; returns the device chain's batches and outputs.  order: the windows' positions in the batch."""
    import torch
    wb, steps = _plan(la, name, slides)
    if order is not None:
        wb, steps = wb.take(order), [_permuted_inputs(s, order) for s in steps]
    d, h = _solver(la, wb, jac, structured), _solver(la, wb, jac, structured)
    d.upload(wb); h.upload(wb)
    st = None if stream is None else C.c_void_p(stream.cuda_stream)
    trail = []
    for k, inputs in enumerate(steps):
        what = f"{name} {jac} structured={structured} slide {k}"
        d.solve_resident(st); h.solve_resident()
        _same_solve(la, d, h, what)
        od, oh = _outs(wb.B), _outs(wb.B, 4)
        dev = _dev(inputs)
        torch.cuda.synchronize()
        d.slide_resident_dev(*dev, out=od, stream=stream)
        h.slide_resident(*inputs, out=oh)
        got, want = _fetch(od), _fetch(oh)
        _same_outputs(got, want, what)
        assert not got[4].any(), (what, got[4])
        now = d.download_batch()
        S.assert_same_tables(now, h.download_batch(), what)
        trail.append((now, got))
    d.solve_resident(st); h.solve_resident()
    _same_solve(la, d, h, f"{name} {jac} structured={structured} last solve")
    d.close(); h.close()
    return trail


def _permuted_inputs(inputs, order):
    pose, ranges, priors, drop = inputs
    return (pose[order], None if ranges is None else tuple(a[order] for a in ranges), None if priors is None else tuple(a[order] for a in priors),
            None if drop is None else drop[order])


# ---- 1. the same tables as the host entry -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,jac,structured", [(n, j, 1) for n in S.CASES for j in ("analytic", "numeric")] + [("plain", "analytic", 0), ("plain", "numeric", 0)])
def test_same_tables_as_the_host_entry(gpu, name, jac, structured):
    import localization_amd as la
    _pair_of_chains(la, name, jac, structured, 3)


# ---- 2. queued cycles ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["plain", "ragged", "zprior"])
def test_three_queued_cycles(gpu, name):
    """(solve_resident, slide_resident_dev) x 3 and a last solve with no host synchronisation, download or mirror read in between (the first
    slide's one-time allocation apart), then ONE synchronise: the bits of the same chain through the host entry"""
    import torch
    import localization_amd as la
    wb, steps = _plan(la, name, 3)
    d, h = _solver(la, wb), _solver(la, wb)
    d.upload(wb); h.upload(wb)
    dev = [_dev(s) for s in steps]
    outs = [_outs(wb.B) for _ in steps]
    torch.cuda.synchronize()
    for k in range(3):
        d.solve_resident()
        d.slide_resident_dev(*dev[k], out=outs[k])
    d.solve_resident()
    torch.cuda.synchronize()
    want = []
    for k in range(3):
        h.solve_resident()
        oh = _outs(wb.B, 4)
        torch.cuda.synchronize()
        h.slide_resident(*steps[k], out=oh)
        want.append(_fetch(oh))
    h.solve_resident()
    for k in range(3):
        got = tuple(t.cpu().numpy() for t in outs[k])
        _same_outputs(got, want[k], f"{name} queued slide {k}")
        assert not got[4].any()
    S.assert_same_tables(d.download_batch(), h.download_batch(), name)
    _same_solve(la, d, h, f"{name} after three queued cycles")
    d.close(); h.close()


# ---- 3. refused windows among admitted ones ------------------------------------------------------------------------------------------------------------
def _diag_rows(p_val):
    out = np.zeros(p_val.shape[:-1] + (36,))
    out[..., ::7] = p_val[..., 12:18]
    return out


@pytest.mark.parametrize("densify", [True, False])
@pytest.mark.parametrize("variant", list(K.CODES))
def test_refused_windows_among_admitted_ones(gpu, variant, densify):
    import torch
    import localization_amd as la
    wb_d, chains, spec = K.tight_batch(la)
    wb_h = K.tight_batch(la)[0]
    if variant == "c":
        K.empty_window(wb_d, 1)
    codes = np.array(K.CODES[variant])
    refused, regular = np.flatnonzero(codes), list(K.REGULAR)
    d, h = _solver(la, wb_d), _solver(la, wb_h)
    d.upload(wb_d); h.upload(wb_h)
    d.solve_resident(); h.solve_resident()
    if not densify:   # a first slide that every non-empty window takes: the handle has its table before the slide under test
        first = K.benign_inputs(wb_h, chains, spec)
        dev = _dev(first)
        torch.cuda.synchronize()
        d.slide_resident_dev(*dev); h.slide_resident(*first)
        d.solve_resident(); h.solve_resident()
    before, x_before = d.download_batch(), _solved(la, d)
    assert (before.p_info is None) == densify
    bad = K.refusing_inputs(before, chains, spec, variant)
    good = K.benign_inputs(h.download_batch(), chains, spec)
    od, oh = _outs(8), _outs(8, 4)
    dev = _dev(bad)
    torch.cuda.synchronize()
    d.slide_resident_dev(*dev, out=od)
    h.slide_resident(*good, out=oh)
    slot, prior, rank, status, admit = _fetch(od)
    want = _fetch(oh)
    print(f"variant {variant} densify {densify}: admit {admit.tolist()} status {status.tolist()}")
    assert admit.tolist() == codes.tolist()
    assert status[refused].tolist() == K.status_of(codes)[refused].tolist()
    assert (slot[refused] == -1).all() and not prior[refused].any() and not rank[refused].any()
    # the refused windows are exactly what they were: every row of every table (used or not), the input estimates, the optimised poses
    after, x_after = d.download_batch(), _solved(la, d)
    for name in CHAIN3_SLIDE_TABLES:
        assert getattr(after, name)[refused].tobytes() == getattr(before, name)[refused].tobytes(), name
    assert x_after.poses[refused].tobytes() == x_before.poses[refused].tobytes()
    assert after.p_info is not None
    if densify:   # the handle has a table from now on, for the refused windows as well: their priors' diagonals
        used = np.arange(after.caps[2])[None, :] < after.counts[refused, 2:3]
        assert after.p_info[refused].tobytes() == np.where(used[..., None], _diag_rows(before.p_val[refused]), 0.0).tobytes()
    else:
        assert after.p_info[refused].tobytes() == before.p_info[refused].tobytes()
    # the regular windows slid as through the host entry
    _same_outputs((slot, prior, rank, status), want, variant, regular)
    ref = h.download_batch()
    for b in regular:
        nv, nr, npr, _ = (int(x) for x in ref.counts[b])
        assert after.counts[b].tolist() == ref.counts[b].tolist()
        for name, n in (("poses", nv), ("r_idx", nr), ("r_val", nr), ("p_idx", npr), ("p_val", npr), ("p_info", npr)):
            assert getattr(after, name)[b, :n].tobytes() == getattr(ref, name)[b, :n].tobytes(), (name, b)
    d.solve_resident(); h.solve_resident()
    _same_solve(la, d, h, f"variant {variant} after the slide", regular)
    d.close(); h.close()


# ---- 4. the lazy mirror -----------------------------------------------------------------------------------------------------------------------------------
def test_a_host_slide_after_a_device_slide(gpu):
    """the host entry admits from the mirror: after a device slide it has to fetch it ("ragged" grows, so a stale mirror misjudges rule 3)"""
    import torch
    import localization_amd as la
    wb, steps = _plan(la, "ragged", 2)
    d, h = _solver(la, wb), _solver(la, wb)
    d.upload(wb); h.upload(wb)
    d.solve_resident(); h.solve_resident()
    dev = _dev(steps[0])
    torch.cuda.synchronize()
    d.slide_resident_dev(*dev); h.slide_resident(*steps[0])
    d.solve_resident(); h.solve_resident()
    d.slide_resident(*steps[1]); h.slide_resident(*steps[1])
    S.assert_same_tables(d.download_batch(), h.download_batch(), "device slide, then host slide")
    d.solve_resident(); h.solve_resident()
    _same_solve(la, d, h, "device slide, then host slide")
    d.close(); h.close()


def _growing_plain(la):
    """the "plain" windows under capacities for seven poses, and the inputs that grow them to seven"""
    _, chains, spec = S.case_batch(la, "plain")
    wb = la.WindowBatch(8, *S.caps_for(7))
    for i, ch in enumerate(chains):
        F.add_chain_poses(wb, i, ch, 0, 6)
    spec["drop"] = np.zeros(8, dtype=np.int32)
    return wb, S.next_inputs(wb, chains, spec)


def test_joint_covariance_sees_the_slid_counts(gpu):
    import torch
    import localization_amd as la
    wb, inputs = _growing_plain(la)
    d = _solver(la, wb)
    d.upload(wb); d.solve_resident()
    dev = _dev(inputs)
    torch.cuda.synchronize()
    d.slide_resident_dev(*dev)
    d.solve_resident()
    B, nvm = wb.B, wb.caps[0]
    t = torch.device("cuda", 0)
    cov = torch.zeros((B, nvm, 36), dtype=torch.float64, device=t); cross = torch.zeros((B, 1, 36), dtype=torch.float64, device=t)
    mask = torch.zeros((B, nvm), dtype=torch.int32, device=t); status = torch.zeros(B, dtype=torch.int32, device=t)
    torch.cuda.synchronize()
    d.joint_covariance_resident(np.array([[0, 6]], dtype=np.int32), None, cov, mask, status, cross)   # the new last slot
    torch.cuda.synchronize()
    assert not status.cpu().numpy().any() and np.isfinite(cross.cpu().numpy()).all()
    with pytest.raises(la.LocalizationAmdError) as e:
        d.joint_covariance_resident(np.array([[0, 7]], dtype=np.int32), None, cov, mask, status, cross)   # one past it
    assert e.value.code == LOC_ERR_INVALID
    d.close()


def test_set_anchors_sees_the_anchor_a_device_slide_introduced(gpu):
    import torch
    import localization_amd as la
    anchors = np.vstack([F.ANCH, [[4.0, 0.0, 1.0], [-4.0, 0.5, 1.5]]])   # eight; the uploaded batch names the first six at most
    wb, steps = _plan(la, "plain", 1)
    pose, (rc, ri, rv), priors, drop = steps[0]
    ri[0, 0, 1] = -1 - 7                                                  # window 0's first new range goes to anchor 7
    rv[0, 0, 0] = np.linalg.norm(pose[0, 9:] - anchors[7])
    d = _solver(la, wb, anchors=anchors)
    d.upload(wb); d.solve_resident()
    dp = C.POINTER(C.c_double)
    admit = _outs(8)
    dev = _dev((pose, (rc, ri, rv), priors, drop))
    torch.cuda.synchronize()
    d.slide_resident_dev(*dev, out=admit)
    assert not _fetch(admit)[4].any()
    assert d.L.loc_window_set_anchors(d.h, 7, anchors.ctypes.data_as(dp)) == LOC_ERR_INVALID
    assert d.L.loc_window_set_anchors(d.h, 8, anchors.ctypes.data_as(dp)) == 0
    d.solve_resident()
    assert np.isfinite(_solved(la, d).result[:, :2]).all()
    d.close()


# ---- 5. batch-level refusals: the host entry's codes, nothing launched or changed ---------------------------------------------------------------------
def _rotation_entry(wb):
    wb.p_info = np.zeros((8, S.NP_MAX, 36)); wb.p_info[:, :, 3 * 6 + 3] = 40.0


def _lever_arm1(wb):
    wb.r_off1 = np.zeros((8, wb.caps[1], 3)); wb.r_off1[3, 0] = (0.1, 0, 0)


def _lever_arm0(wb):
    wb.r_val[1, 0, 2:5] = (0.05, 0, 0)


@pytest.mark.parametrize("how", ["option_0", "unsolved", "six_dof", "endpoint1", "rotation_table", "null_new_pose"])
def test_refused_batches(gpu, how):
    import torch
    import localization_amd as la
    code = LOC_ERR_INVALID if how in ("option_0", "unsolved", "null_new_pose") else LOC_ERR_UNSUPPORTED
    wb, steps = _plan(la, "plain", 1)
    change = {"six_dof": _lever_arm0, "endpoint1": _lever_arm1, "rotation_table": _rotation_entry}.get(how)
    if change is not None:
        change(wb)
    d, h = _solver(la, wb, slide=0 if how == "option_0" else 1), _solver(la, wb, slide=0 if how == "option_0" else 1)
    for s in (d, h):
        s.upload(wb)
        if how != "unsolved":
            s.solve_resident()
    before = d.download_batch()
    out = _outs(8)
    pose, ranges, priors, drop = _dev(steps[0])
    torch.cuda.synchronize()
    with pytest.raises(la.LocalizationAmdError) as e:
        d.slide_resident_dev(None if how == "null_new_pose" else pose, ranges, priors, drop, out=out)
    assert e.value.code == code, (e.value, code)
    if how != "null_new_pose":   # the host entry's code for the same handle state
        with pytest.raises(la.LocalizationAmdError) as eh:
            h.slide_resident(*steps[0])
        assert eh.value.code == code
    for t in _fetch(out):
        assert (t == POISON).all()
    after = d.download_batch()
    for name in CHAIN3_SLIDE_TABLES:
        assert getattr(after, name).tobytes() == getattr(before, name).tobytes(), name
    assert (after.p_info is None) == (before.p_info is None) and (after.p_info is None or after.p_info.tobytes() == before.p_info.tobytes())
    d.close(); h.close()


# ---- 6. a second stream, and another position in the batch ------------------------------------------------------------------------------------------------
def test_a_second_stream_and_another_position_give_the_same_bits(gpu):
    import torch
    import localization_amd as la
    base = _pair_of_chains(la, "zprior", "numeric", 1, 2)
    other = _pair_of_chains(la, "zprior", "numeric", 1, 2, stream=torch.cuda.Stream())
    order = np.array([6, 3, 0, 5, 2, 7, 4, 1])
    moved = _pair_of_chains(la, "zprior", "numeric", 1, 2, order=order)
    for (a, oa), (b, ob), (c, oc) in zip(base, other, moved):
        S.assert_same_tables(b, a, "second stream")
        S.assert_same_tables(c, a.take(order), "another position")
        for x, y, z in zip(oa, ob, oc):
            assert x.tobytes() == y.tobytes() and x[order].tobytes() == z.tobytes()
