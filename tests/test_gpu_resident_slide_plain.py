"""The resident plain-drop slide of 6-DoF chain windows (loc_window_slide_plain_resident_dev; DESIGN.md §2, "The plain drop for 6-DoF chain
windows"): slot 0 goes with every factor on it, nothing is carried, the newest pose and its factors are appended — in the device tables of the
verdicts CHAIN, WAVE6 and WAVE6S.  The yardstick is the rule in numpy (tests/_slide_plain_ref.py), BIT FOR BIT: the slide moves rows and computes
nothing, so no tolerance is involved anywhere but against the oracle, where tests/test_gpu_wave6_parity.py's applies (analytic mode: 1e-7 on
every pose entry, 1e-6 relative on chi2).  Eight windows per case; the refusals are held to the rule without a GPU by
tests/test_resident_slide_plain_cpu.py.

Every case is run ONCE (_run_case) and shared by the tests that read it.  torch copies the inputs on ITS stream and the handle's stream does not
wait for it: every test synchronises before it hands pointers over."""
import ctypes as C
import functools

import numpy as np
import pytest

import _slide_plain_ref as P

pytestmark = pytest.mark.gpu

LOC_ERR_INVALID, LOC_ERR_UNSUPPORTED = -1, -5
POISON = -77
GENERAL = "window_lm_kernel"


def _solver(la, wb, jac="analytic", slide=1):
    s = la.WindowSolver(P.ANCH, wb.B, *wb.caps, jacobian=jac)
    s.set_option("resident_slide", slide)
    return s


def _dev(inputs):
    """(new_pose, new_ranges, new_priors, new_se3, drop_oldest) as torch device tensors, in the order of slide_plain_resident_dev's arguments"""
    import torch
    d = torch.device("cuda", 0)
    t = lambda a, dt: torch.from_numpy(np.array(a, dtype=dt)).to(d)   # (a copy: the inputs stay the caller's)
    pose, ranges, priors, se3, drop = inputs
    B = len(pose)
    return (t(pose, np.float64), (t(ranges[0], np.int32), t(ranges[1], np.int32), t(ranges[2], np.float64)),
            (t(priors[0], np.int32), t(priors[1], np.float64)), (t(se3[0], np.int32), t(se3[1], np.int32), t(se3[2], np.float64)),
            None if drop is None else t(np.broadcast_to(drop, (B,)), np.int32))


def _outs(B):
    """(status, admit) poisoned"""
    import torch
    return tuple(torch.full((B,), POISON, dtype=torch.int32, device=torch.device("cuda", 0)) for _ in range(2))


def _fetch(out):
    import torch
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _solved(la, s):
    wb = la.WindowBatch(s._resident, *s.caps)
    s.download(wb)
    return wb


def _with_poses(la, wb, poses):
    out = wb.copy()
    out.poses[:] = poses
    return out


def _same_solution(x, y, counts, what):
    """two downloaded solves: optimised poses (the used slots) and results, byte for byte"""
    used = np.arange(x.caps[0])[None, :] < counts[:, :1]
    assert x.poses[used].tobytes() == y.poses[used].tobytes(), (what, np.abs(x.poses[used] - y.poses[used]).max())
    assert x.result.tobytes() == y.result.tobytes(), (what, x.result, y.result)


def _slide(s, dev, out=None, stream=None):
    pose, ranges, priors, se3, drop = dev
    s.slide_plain_resident_dev(pose, ranges, priors, se3, drop, out=out, stream=stream)


@functools.lru_cache(maxsize=None)
def _run_case(name, jac="analytic"):
    """upload, solve_resident, then three slides with a resident solve after each; per slide: the downloaded tables, the poses array, the
    outputs, the numpy-slid batch, the slid handle's solve and a fresh handle's solve of the numpy-slid batch, and both kernel kinds"""
    import torch
    import localization_amd as la
    wb, streams, spec = P.case_batch(la, name)
    s = _solver(la, wb, jac)
    s.upload(wb); s.solve_resident()
    first_kind = s.last_kernel_kind()
    ref, steps = wb, []
    for k in range(P.SLIDES):
        inputs = P.next_inputs(ref, streams, spec)
        x = _solved(la, s)
        want = P.slide_plain_ref(la, _with_poses(la, ref, x.poses), *inputs)
        dev, out = _dev(inputs), _outs(wb.B)
        torch.cuda.synchronize()
        _slide(s, dev, out)
        status, admit = _fetch(out)
        tables, poses_out = s.download_batch(), _solved(la, s).poses.copy()
        s.solve_resident()
        fresh = _solver(la, want, jac)
        fresh.upload(want); fresh.solve_resident()
        steps.append(dict(status=status, admit=admit, tables=tables, poses_out=poses_out, want=want, slid=_solved(la, s), fresh=_solved(la, fresh),
                          kinds=(s.last_kernel_kind(), fresh.last_kernel_kind())))
        fresh.close()
        ref = want
    s.close()
    return first_kind, steps


# ---- 1. the re-pack, bit for bit ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(P.CASES))
def test_repack_bit_for_bit(gpu, name):
    first_kind, steps = _run_case(name)
    kernel = P.CASES[name].get("kernel")
    assert kernel is None or first_kind == kernel, (first_kind, kernel)
    if name == "long":   # 159 range, 80 prior and 78 EdgeSE3 rows: two or three 64-row steps in every table
        assert steps[0]["want"].counts[:, 1:].tolist() == [[159, 80, 78]] * 8
    for k, st in enumerate(steps):
        what = f"{name} slide {k}"
        assert not st["admit"].any() and not st["status"].any(), (what, st["admit"], st["status"])
        P.assert_same_tables(st["tables"], st["want"], what)   # (the next solve's input estimates among them)
        used = np.arange(st["want"].caps[0])[None, :] < st["want"].counts[:, :1]
        assert st["poses_out"][used].tobytes() == st["want"].poses[used].tobytes(), what
        assert st["tables"].p_info is None, what


# ---- 2. the slid batch solves as an uploaded one -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(P.CASES))
def test_slid_batch_solves_as_an_uploaded_one(gpu, name):
    first_kind, steps = _run_case(name)
    for k, st in enumerate(steps):
        what = f"{name} solve after slide {k}"
        assert st["kinds"][0] == st["kinds"][1] == first_kind, (what, st["kinds"], first_kind)
        if name == "twist":
            assert (st["want"].counts[:, 3] > 0).all()
        _same_solution(st["slid"], st["fresh"], st["want"].counts, what)


# ---- 3. against the oracle ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["imu", "twist"])
def test_slid_windows_against_the_oracle(gpu, name):
    from oracle import oracle as O
    from _oracle_window import oracle_solve_instance
    _, steps = _run_case(name)
    for k, st in enumerate(steps):
        for i in range(8):
            nv = int(st["want"].counts[i, 0])
            poses, chi, _ = oracle_solve_instance(st["want"], i, P.ANCH, jac_mode=O.JAC_ANALYTIC)
            d = np.abs(st["slid"].poses[i, :nv] - poses).max()
            print(f"{name} slide {k} window {i}: |dx| {d:.3e} chi2 {st['slid'].result[i, 0]:.9g} oracle {chi:.9g}")
            assert d < 1e-7, (name, k, i, d)
            assert abs(st["slid"].result[i, 0] - chi) <= 1e-6 * max(1.0, abs(chi)), (name, k, i, st["slid"].result[i, 0], chi)


# ---- 4. refusals leave a window alone ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(P.REFUSALS))
def test_a_refused_window_is_left_alone(gpu, variant):
    import torch
    import localization_amd as la
    case, code = P.REFUSALS[variant]
    wb, streams, spec = P.refusal_batch(la, variant)
    s = _solver(la, wb)
    s.upload(wb); s.solve_resident()
    assert s.last_kernel_kind() == P.CASES[case]["kernel"]
    before, x = s.download_batch(), _solved(la, s)
    _, refusing = P.refusing_inputs(wb, streams, spec, variant)
    dev, out = _dev(refusing), _outs(8)
    torch.cuda.synchronize()
    _slide(s, dev, out)
    status, admit = _fetch(out)
    print(f"variant {variant}: admit {admit.tolist()} status {status.tolist()}")
    codes = np.zeros(8, dtype=int); codes[P.REFUSED] = code
    assert admit.tolist() == codes.tolist()
    assert status.tolist() == P.status_of(codes).tolist()
    after, x_after = s.download_batch(), _solved(la, s)
    for name in P.TABLES:   # every row of every table (used or not) and the next solve's input estimates
        assert getattr(after, name)[P.REFUSED].tobytes() == getattr(before, name)[P.REFUSED].tobytes(), name
    assert x_after.poses[P.REFUSED].tobytes() == x.poses[P.REFUSED].tobytes()
    want = P.slide_plain_ref(la, _with_poses(la, wb, x.poses), *refusing, refused=(P.REFUSED,))
    others = [b for b in range(8) if b != P.REFUSED]
    P.assert_same_tables(after, want, variant, others)
    used = np.arange(wb.caps[0])[None, :] < want.counts[:, :1]
    used[P.REFUSED] = False
    assert x_after.poses[used].tobytes() == want.poses[used].tobytes()
    assert after.p_info is None
    s.close()


# ---- 5. host refusals: nothing launched or changed -----------------------------------------------------------------------------------------------------------
def _chain3_batch(la):
    """the "imu" windows without anything that turns a pose: identity rotations, no lever arm, no rotation information"""
    wb, streams, spec = P.case_batch(la, "imu")
    wb.poses[:, :, :9] = np.eye(3).reshape(9)
    wb.r_val[:, :, 2:] = 0.0
    wb.p_val[:, :, :9] = np.eye(3).reshape(9); wb.p_val[:, :, 15:] = 0.0; wb.p_val[:, :, 12:15] = 4.0
    return wb, streams, spec


def _forest_batch(la):
    """the "twist" windows with a key-frame EdgeSE3 from slot 0 to slot 3 in the place of their last one: no chain"""
    wb, streams, spec = P.case_batch(la, "twist")
    wb.s_idx[:, 4, :2] = (0, 3)
    return wb, streams, spec


def _endpoint1_batch(la):
    wb, streams, spec = P.case_batch(la, "imu")
    wb.r_off1 = np.zeros((8, wb.caps[1], 3)); wb.r_off1[3, 0] = (0.1, 0, 0)
    return wb, streams, spec


def _table_batch(la):
    wb, streams, spec = P.case_batch(la, "imu")
    wb.p_info = np.zeros((8, wb.caps[2], 36)); wb.p_info[:, :, ::7] = wb.p_val[:, :, 12:]
    return wb, streams, spec


HOST_REFUSALS = {"option_off": LOC_ERR_INVALID, "unsolved": LOC_ERR_INVALID, "null_new_pose": LOC_ERR_INVALID, "null_array": LOC_ERR_INVALID,
                 "chain3": LOC_ERR_UNSUPPORTED, "forest": LOC_ERR_UNSUPPORTED, "endpoint1": LOC_ERR_UNSUPPORTED, "table": LOC_ERR_UNSUPPORTED}


@pytest.mark.parametrize("how", list(HOST_REFUSALS))
def test_refused_batches(gpu, how):
    import torch
    import localization_amd as la
    make = {"chain3": _chain3_batch, "forest": _forest_batch, "endpoint1": _endpoint1_batch, "table": _table_batch}.get(how, lambda la: P.case_batch(la, "imu"))
    wb, streams, spec = make(la)
    s = _solver(la, wb, slide=0 if how == "option_off" else 1)
    s.upload(wb)
    if how != "unsolved":
        s.solve_resident()
    before = s.download_batch()
    pose, ranges, priors, se3, drop = _dev(P.next_inputs(wb, streams, spec))
    if how == "null_new_pose":
        pose = None
    if how == "null_array":
        ranges = (ranges[0], None, ranges[2], ranges[1].shape[1])
    out = _outs(8)
    torch.cuda.synchronize()
    with pytest.raises(la.LocalizationAmdError) as e:
        s.slide_plain_resident_dev(pose, ranges, priors, se3, drop, out=out)
    assert e.value.code == HOST_REFUSALS[how], (e.value, HOST_REFUSALS[how])
    if how == "chain3":
        assert "loc_window_slide_resident" in str(e.value)
    for t in _fetch(out):
        assert (t == POISON).all()
    after = s.download_batch()
    for name in P.TABLES:
        assert getattr(after, name).tobytes() == getattr(before, name).tobytes(), name
    assert (after.p_info is None) == (before.p_info is None) and (after.p_info is None or after.p_info.tobytes() == before.p_info.tobytes())
    s.close()


# ---- 6. queued cycles -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["imu", "twist"])
def test_three_queued_cycles(gpu, name):
    """(solve_resident, slide) x 3 and a last solve on ONE non-default stream with no host synchronisation, download or mirror read in between,
    then one synchronise: the bits of the step-by-step run"""
    import torch
    import localization_amd as la
    _, steps = _run_case(name)
    wb, streams, spec = P.case_batch(la, name)
    counts, inputs = wb.counts.copy(), []
    for k in range(P.SLIDES):   # (these cases drop in every slide: the counts a slide's inputs are made for do not change)
        inputs.append(P.next_inputs(wb, streams, spec))
    assert np.array_equal(counts[:, 0], steps[-1]["want"].counts[:, 0])
    stream = torch.cuda.Stream()
    st = C.c_void_p(stream.cuda_stream)
    s = _solver(la, wb)
    s.upload(wb)
    dev = [_dev(x) for x in inputs]   # (kept alive until the stream has passed the calls)
    outs = [_outs(8) for _ in inputs]
    torch.cuda.synchronize()
    for k in range(P.SLIDES):
        s.solve_resident(st)
        _slide(s, dev[k], outs[k], stream)
    s.solve_resident(st)
    torch.cuda.synchronize()
    for o in outs:
        status, admit = (t.cpu().numpy() for t in o)
        assert not status.any() and not admit.any()
    P.assert_same_tables(s.download_batch(), steps[-1]["want"], f"{name} after three queued cycles")
    _same_solution(_solved(la, s), steps[-1]["slid"], steps[-1]["want"].counts, f"{name} after three queued cycles")
    s.close()


# ---- 7. position independence -------------------------------------------------------------------------------------------------------------------------------------
def test_another_position_gives_the_same_bits(gpu):
    import torch
    import localization_amd as la
    wb, streams, spec = P.case_batch(la, "twist")
    for name in P.TABLES:
        getattr(wb, name)[5] = getattr(wb, name)[1]
    inputs = P.next_inputs(wb, streams, spec)
    pose, ranges, priors, se3, drop = inputs
    for a in (pose,) + ranges + priors + se3:
        a[5] = a[1]
    s = _solver(la, wb)
    s.upload(wb); s.solve_resident()
    dev = _dev(inputs)
    torch.cuda.synchronize()
    _slide(s, dev)
    after, x = s.download_batch(), _solved(la, s)
    assert after.counts[1, 0] == 6 and after.counts[1, 3] == 5
    for name in P.TABLES:
        assert getattr(after, name)[5].tobytes() == getattr(after, name)[1].tobytes(), name
    assert x.poses[5].tobytes() == x.poses[1].tobytes()
    s.close()


# ---- 8. the neighbours on the slid batch -------------------------------------------------------------------------------------------------------------------------
def _neighbours(la, s, caps, prune):
    """covariance_resident, edge_chi2_resident, joint_covariance_resident with pairs (a mirror read) — and, with prune, prune_resident followed
    by a solve — of a handle at its solved poses, as host arrays"""
    import torch
    t = torch.device("cuda", 0)
    B, (nvm, nrm, npm, nsm) = 8, caps
    z = lambda shape, dt=torch.float64: torch.zeros(shape, dtype=dt, device=t)
    cov, mask, status = z((B, nvm, 36)), z((B, nvm), torch.int32), z((B,), torch.int32)
    chi = (z((B, nrm)), z((B, npm)), z((B, max(nsm, 1))), z((B,)), z((B,), torch.int32))
    jcov, jmask, jstatus, cross = z((B, nvm, 36)), z((B, nvm), torch.int32), z((B,), torch.int32), z((B, 2, 36))
    removed, n_removed = z((B, nrm), torch.int32), z((B,), torch.int32)
    torch.cuda.synchronize()
    s.covariance_resident(cov, mask, status)
    s.edge_chi2_resident(*chi)
    s.joint_covariance_resident(np.array([[0, 5], [4, 5]], dtype=np.int32), None, jcov, jmask, jstatus, cross)
    got = [cov, mask, status, *chi, jcov, jmask, jstatus, cross]
    if prune:
        s.prune_resident(0.2, 4, removed, n_removed)
        s.solve_resident()
        got += [removed, n_removed]
    torch.cuda.synchronize()
    got = [x.cpu().numpy() for x in got]
    if prune:
        x = _solved(la, s)
        got += [x.poses, x.result]
    return got


def test_the_neighbours_see_the_slid_batch(gpu):
    import torch
    import localization_amd as la
    wb, streams, spec = P.case_batch(la, "imu")
    s = _solver(la, wb)
    s.upload(wb); s.solve_resident()
    inputs = P.next_inputs(wb, streams, spec)
    want = P.slide_plain_ref(la, _with_poses(la, wb, _solved(la, s).poses), *inputs)
    dev = _dev(inputs)
    torch.cuda.synchronize()
    _slide(s, dev)
    s.solve_resident()
    fresh = _solver(la, want)
    fresh.upload(want); fresh.solve_resident()
    a, b = _neighbours(la, s, wb.caps, True), _neighbours(la, fresh, wb.caps, True)
    names = ["cov", "mask", "status", "r_chi2", "p_chi2", "s_chi2", "total", "active", "joint cov", "joint mask", "joint status", "cross", "removed", "n_removed",
             "poses after the removal", "result after the removal"]
    used = np.arange(wb.caps[0])[None, :] < want.counts[:, :1]
    for name, x, y in zip(names, a, b):
        if name in ("cov", "mask", "joint cov", "joint mask", "poses after the removal"):   # (per pose slot: the used slots)
            x, y = x[used], y[used]
        assert x.tobytes() == y.tobytes(), name
    assert a[13].sum() > 0, "the removal has to remove something for the next slide to carry"
    # a removed row (information exactly 0.0) travels through the next slide as it is
    pruned = s.download_batch()
    assert ((pruned.r_val[:, :, 1] == 0.0) & (a[12] == 1)).sum() == a[13].sum()
    nxt = P.next_inputs(want, streams, spec)
    want2 = P.slide_plain_ref(la, _with_poses(la, pruned, _solved(la, s).poses), *nxt)
    kept_zero = sum(int((want2.r_val[b, :int(want2.counts[b, 1]), 1] == 0.0).sum()) for b in range(8))
    assert kept_zero > 0
    dev = _dev(nxt)
    torch.cuda.synchronize()
    _slide(s, dev)
    P.assert_same_tables(s.download_batch(), want2, "the slide after a removal")
    s.close(); fresh.close()
