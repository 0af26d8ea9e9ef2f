"""A resident batch from the caller's DEVICE arrays (loc_window_upload_dev; window_admit_kernel.hip; DESIGN.md §2, "Upload from device arrays").
The yardstick is loc_window_upload of the same arrays on a second handle, BIT FOR BIT: the call moves tables and classifies, it computes no
number a solve reads, so there is no tolerance anywhere.  The admission codes are held to the numpy rule of tests/_window_structure_model.py
(the rule itself, window by window, is held to window_structure.cpp without a GPU by tests/test_window_admit_cpu.py).

Batches of 3 to 24 windows.  torch copies the inputs on ITS stream and the handle's stream does not wait for it: every test synchronises before
it hands pointers over (but the stream-order test, which is about exactly that)."""
import ctypes as C
import types

import numpy as np
import pytest

import _slide_plain_ref as P
import _window_structure_model as M

pytestmark = pytest.mark.gpu

LOC_ERR_INVALID = -1
TABLES = P.TABLES
GENERAL, CHAIN, WAVE3, WAVE6, WAVE6S = "window_lm_kernel", "chain_lm_kernel", "wave3_lm_kernel", "wave6_lm_kernel", "wave6_lm_kernel<SE3>"
WORDS = {1: "counts exceed capacities", 2: "range edge vertex index", 3: "range edge couples poses further apart than bw_max", 4: "prior edge vertex index",
         5: "SE3 edge vertex index", 6: "SE3 edge couples poses further apart than bw_max"}


def _dev(wb):
    """the eight tables as torch device tensors (copies: the batch stays the caller's)"""
    import torch
    d = torch.device("cuda", 0)
    return [torch.from_numpy(np.ascontiguousarray(getattr(wb, name))).to(d) for name in TABLES]


def _solver(la, wb, jac="analytic", slide=0, bw_max=-1, **options):
    s = la.WindowSolver(P.ANCH, wb.B, *wb.caps, jacobian=jac, bw_max=bw_max)
    s.set_option("resident_slide", slide)
    for k, v in options.items():
        s.set_option(k, v)
    return s


def _upload_dev(s, wb, admit=None, stream=None):
    import torch
    dev = _dev(wb)
    torch.cuda.synchronize()
    s.upload_dev(*dev, admit=admit, stream=stream)
    return dev


def _solved(la, s):
    wb = la.WindowBatch(s._resident, *s.caps)
    s.download(wb)
    return wb


def _same_solution(x, y, counts, what):
    used = np.arange(x.caps[0])[None, :] < counts[:, :1]
    assert x.poses[used].tobytes() == y.poses[used].tobytes(), (what, np.abs(x.poses[used] - y.poses[used]).max())
    assert x.result.tobytes() == y.result.tobytes(), (what, x.result, y.result)


def _append_range(wb, i, v0, v1, like):
    """one more range row on window i, with the values of its row `like`"""
    e = int(wb.counts[i, 1])
    assert e < wb.caps[1]
    wb.r_idx[i, e] = (v0, v1); wb.r_val[i, e] = wb.r_val[i, like]
    wb.counts[i, 1] = e + 1


def _pair_row(wb, i, key2):
    """the row of window i's range between poses key2 - 1 and key2"""
    rows = [e for e in range(int(wb.counts[i, 1])) if wb.r_idx[i, e, 1] >= 0 and max(wb.r_idx[i, e]) == key2]
    assert rows, (i, key2)
    return rows[0]


def _chain3(la, spare=(0, 0, 0)):
    """the "imu" windows without anything that turns a pose: identity rotations, no lever arm, no rotation information"""
    wb = P.case_batch(la, "imu", spare)[0]
    wb.poses[:, :, :9] = np.eye(3).reshape(9)
    wb.r_val[:, :, 2:] = 0.0
    wb.p_val[:, :, :9] = np.eye(3).reshape(9); wb.p_val[:, :, 15:] = 0.0; wb.p_val[:, :, 12:15] = 4.0
    return wb


def _batch_of(la, kind):
    """eight windows of a verdict: (batch, the kernel a resident solve of it runs on, the same under a batch threshold of 1, control) —
    control: None, or (options, kernels): loc_window_upload on a handle with these options answers one of these kernels for the batch"""
    if kind == "chain3":
        return _chain3(la), WAVE3, "chain3_lm_kernel", None
    if kind == "wave6":
        return P.case_batch(la, "imu")[0], WAVE6, CHAIN, None
    if kind == "wave6s":
        return P.case_batch(la, "twist")[0], WAVE6S, CHAIN, None
    if kind == "chain":                       # two ranges on one pair of window 5, the second one after the anchor rows of the pair's later pose
        wb = P.case_batch(la, "imu", (1, 0, 0))[0]
        nv = int(wb.counts[5, 0])
        assert max(wb.r_idx[5, int(wb.counts[5, 1]) - 1]) == nv - 1
        _append_range(wb, 5, nv - 1, nv - 2, _pair_row(wb, 5, nv - 1))
        return wb, GENERAL, CHAIN, None
    if kind == "general":                     # a loop edge in window 2
        wb = P.case_batch(la, "imu", (1, 0, 0))[0]
        _append_range(wb, 2, 0, int(wb.counts[2, 0]) - 1, _pair_row(wb, 2, 1))
        return wb, GENERAL, GENERAL, None
    if kind == "forest":                      # tests/test_gpu_tree_parity.py's key-frame stars: ONE topology, EdgeSE3 rows 0 - {1, 2, 3} and 3 - {4 .. 7}, an anchor range per pose
        import test_gpu_tree_parity as F
        assert F.ANCH.tobytes() == P.ANCH.tobytes()
        wb = F._forest_batch(la, np.random.default_rng(77), 8, 8, 4, False)
        assert all(wb.r_idx[i].tobytes() == wb.r_idx[0].tobytes() and wb.s_idx[i].tobytes() == wb.s_idx[0].tobytes() for i in range(8))
        assert sorted(tuple(sorted(e)) for e in wb.s_idx[0, :7, :2].tolist()) == [(0, 1), (0, 2), (0, 3), (3, 4), (3, 5), (3, 6), (3, 7)] and (wb.r_idx[0, :8, 1] < 0).all()
        return wb, GENERAL, GENERAL, (dict(chain_min_batch=1), ("tree_wave_kernel", "tree_lm_kernel"))
    assert kind == "arrow"                    # translation-only, the last pose a border every other pose ranges to
    wb = _chain3(la, (4, 0, 0))
    for i in range(wb.B):
        nv = int(wb.counts[i, 0])
        for v in range(min(nv - 2, 4)):
            _append_range(wb, i, v, nv - 1, _pair_row(wb, i, nv - 1))
    return wb, GENERAL, GENERAL, (dict(arrow3=1), ("arrow3_lm_kernel",))


# ---- 1. the same state as the host upload ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jac", ["analytic", "numeric"])
@pytest.mark.parametrize("kind", ["chain3", "wave6", "wave6s", "chain", "general", "forest", "arrow"])
def test_same_state_as_the_host_upload(gpu, kind, jac):
    import localization_amd as la
    wb, kernel, kernel_at_1, control = _batch_of(la, kind)
    if control:                               # the batch IS what its name says: the host upload takes the structured kernel for it when allowed to
        c = _solver(la, wb, jac, **control[0])
        c.upload(wb); c.solve_resident()
        assert c.last_kernel_kind() in control[1], (kind, c.last_kernel_kind())
        c.close()
    a, h = _solver(la, wb, jac), _solver(la, wb, jac, tree=0, arrow3=0)
    _upload_dev(a, wb); h.upload(wb)
    for s in (a, h):
        s.solve_resident()
    assert a.last_kernel_kind() == h.last_kernel_kind() == kernel
    _same_solution(_solved(la, a), _solved(la, h), wb.counts, kind)
    for s in (a, h):                          # the verdict itself, past the batch threshold: CHAIN and GENERAL run on one kernel below it
        s.L.loc_window_set_chain_threshold(s.h, 1)
        s.solve_resident()
    assert a.last_kernel_kind() == h.last_kernel_kind() == kernel_at_1
    _same_solution(_solved(la, a), _solved(la, h), wb.counts, kind + " at threshold 1")
    P.assert_same_tables(a.download_batch(), h.download_batch(), kind)
    a.close(); h.close()


def _long_chain3(la):
    """three translation-only chain windows under nv_max 40; the middle one has 40 poses, 79 range rows and 40 priors, so that every value
    loop of the admit pass (256 elements a step: 21 poses, 51 range rows, 14 priors) takes a second step with the verdict still open"""
    rng = np.random.default_rng(40)
    wb = la.WindowBatch(3, 40, 79, 40, 0)
    for i, nv in enumerate((6, 40, 9)):
        xs = np.cumsum(rng.normal(0.0, 0.05, (nv, 3)), axis=0) + (0.5, 0.2, 1.0)
        for k in range(nv):
            wb.add_pose(i, xs[k] + rng.normal(0.0, 0.01, 3))
            if k:
                wb.add_range(i, k - 1, k, float(np.linalg.norm(xs[k] - xs[k - 1])), P.SMOOTH_INFO)
            an = int(rng.integers(4))
            wb.add_range(i, k, an, float(np.linalg.norm(xs[k] - P.ANCH[an])), P.RANGE_INFO, anchor=True)
            wb.add_prior(i, k, xs[k], np.eye(3), info_diag=(4.0, 4.0, 4.0, 0.0, 0.0, 0.0))
    assert wb.counts[1].tolist() == [40, 79, 40, 0]
    return wb


# (table, row, column, value) in window 1, each beyond the first 256 elements of its table; does the batch stay translation-only
LONG_VARIANTS = {
    "as built": (None, True),
    "-0.0 in a pose's rotation": (("poses", 35, 1, -0.0), False),
    "-0.0 in the last pose's rotation": (("poses", 39, 7, -0.0), False),
    "-0.0 in a lever arm": (("r_val", 70, 3, -0.0), True),
    "a lever arm": (("r_val", 78, 4, 1e-300), False),
    "-0.0 in a prior's measurement rotation": (("p_val", 30, 3, -0.0), False),
    "-0.0 as a prior's rotation information": (("p_val", 30, 16, -0.0), True),
    "a prior's rotation information": (("p_val", 39, 17, 1e-300), False),
}


@pytest.mark.parametrize("variant", list(LONG_VARIANTS))
def test_translation_only_by_bits_and_by_value_beyond_the_first_step(gpu, variant):
    import localization_amd as la
    wb = _long_chain3(la)
    change, translation_only = LONG_VARIANTS[variant]
    if change:
        table, row, column, value = change
        assert row * {"poses": 12, "r_val": 5, "p_val": 18}[table] + column >= 256
        getattr(wb, table)[1, row, column] = value
        assert np.signbit(getattr(wb, table)[1, row, column]) == np.signbit(value)
    a, h = _solver(la, wb), _solver(la, wb)
    _upload_dev(a, wb); h.upload(wb)
    for s in (a, h):
        s.solve_resident()
    assert a.last_kernel_kind() == h.last_kernel_kind(), variant
    assert (a.last_kernel_kind() == WAVE3) == translation_only, (variant, a.last_kernel_kind())
    _same_solution(_solved(la, a), _solved(la, h), wb.counts, variant)
    a.close(); h.close()


# ---- 2. the 64-row step boundaries ----------------------------------------------------------------------------------------------------------------------
def _step_window(la, se3, extra_pose=63):
    """three windows under nv_max 64; the middle one has 64 poses, 130 range rows, 70 priors and (se3) 66 EdgeSE3 rows — ordered, with lever arms;
    range row 2 k - 1 joins poses k - 1 and k, row 2 k is pose k's anchor range: rows 63 and 64 are pose 32's pair and anchor row.  Pose
    extra_pose has three anchor ranges more, right behind its own"""
    rng = np.random.default_rng(64)
    wb = la.WindowBatch(3, 64, 130, 70, 66 if se3 else 0)
    rot = lambda a: np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    for i, nv in enumerate((5, 64, 7)):
        xs = np.cumsum(rng.normal(0.0, 0.05, (nv, 3)), axis=0) + (0.5, 0.2, 1.0)
        yaw = np.cumsum(rng.normal(0.0, 0.02, nv))
        for k in range(nv):
            wb.add_pose(i, xs[k] + rng.normal(0.0, 0.01, 3), rot(yaw[k]))
            if k:
                wb.add_range(i, k - 1, k, float(np.linalg.norm(xs[k] - xs[k - 1])), P.SMOOTH_INFO)
                if se3:
                    wb.add_se3(i, k - 1, k, rot(yaw[k - 1]).T @ (xs[k] - xs[k - 1]), rot(yaw[k] - yaw[k - 1]), np.eye(6) * 50.0)
            an = int(rng.integers(4))
            wb.add_range(i, k, an, float(np.linalg.norm(xs[k] + rot(yaw[k]) @ P.LEVER - P.ANCH[an])), P.RANGE_INFO, off=P.LEVER, anchor=True)
            wb.add_prior(i, k, xs[k], rot(yaw[k]), info_diag=P.IMU_INFO)
            for _ in range(3 if nv == 64 and k == extra_pose else 0):
                wb.add_range(i, k, 1, float(np.linalg.norm(xs[k] + rot(yaw[k]) @ P.LEVER - P.ANCH[1])), P.RANGE_INFO, off=P.LEVER, anchor=True)
        if nv == 64:
            for _ in range(6):
                wb.add_prior(i, 63, xs[63], rot(yaw[63]), info_diag=P.Z_INFO)
            for _ in range(3 if se3 else 0):
                wb.add_se3(i, 62, 63, rot(yaw[62]).T @ (xs[63] - xs[62]), rot(yaw[63] - yaw[62]), np.eye(6) * 50.0)
    assert wb.counts[1].tolist() == [64, 130, 70, 66 if se3 else 0]
    assert wb.r_idx[1, 63].tolist() == [31, 32] and wb.r_idx[1, 64, 0] == 32 and wb.r_idx[1, 64, 1] < 0
    return wb


def _kinds_and_solutions(la, wb, what):
    """upload_dev against upload: the kernel of a resident solve at a batch threshold of 1 (CHAIN and GENERAL differ there), the same bits"""
    a, h = _solver(la, wb, chain_min_batch=1), _solver(la, wb, chain_min_batch=1, tree=0, arrow3=0)
    _upload_dev(a, wb); h.upload(wb)
    for s in (a, h):
        s.solve_resident()
    kinds = a.last_kernel_kind(), h.last_kernel_kind()
    _same_solution(_solved(la, a), _solved(la, h), wb.counts, what)
    a.close(); h.close()
    assert kinds[0] == kinds[1], (what, kinds)
    return kinds[0]


def test_an_ordering_violation_between_rows_63_and_64(gpu):
    import localization_amd as la
    base = _step_window(la, True)
    assert _kinds_and_solutions(la, base, "the ordered window") == CHAIN
    r = base.copy()
    r.r_idx[1, 64] = (31, -1)                                 # pose 31's anchor range behind pose 32's pair row
    p = base.copy()
    p.p_idx[1, 64] = 62                                       # rows 63 .. 69 are on pose 63
    s = base.copy()
    s.s_idx[1, 64, :2] = (61, 62)                             # rows 62 .. 65 join poses 62 and 63
    for name, wb in (("ranges", r), ("priors", p), ("EdgeSE3", s)):
        assert _kinds_and_solutions(la, wb, name) == GENERAL, name
    inside = base.copy()
    inside.p_idx[1, 63] = 62; inside.p_idx[1, 62] = 63        # the same inside a step, and the step's first row against the carried value
    assert _kinds_and_solutions(la, inside, "inside a step") == GENERAL


def test_a_duplicated_pair_across_rows_63_and_64(gpu):
    import localization_amd as la
    base = _step_window(la, False)
    for wb, kernel in ((base, WAVE6), (None, GENERAL)):
        if wb is None:
            wb = base.copy()
            wb.r_idx[1, 64] = (32, 31)                        # the pair of row 63 again: the verdict is CHAIN, which 3 windows solve on the general kernel
        a, h = _solver(la, wb), _solver(la, wb)
        _upload_dev(a, wb); h.upload(wb)
        for s in (a, h):
            s.solve_resident()
        assert a.last_kernel_kind() == h.last_kernel_kind() == kernel
        _same_solution(_solved(la, a), _solved(la, h), wb.counts, kernel)
        a.close(); h.close()
    assert _kinds_and_solutions(la, wb, "the duplicated pair at threshold 1") == CHAIN
    far = _step_window(la, False, extra_pose=32)              # ... and with anchor rows between the two: rows 63 and 66
    assert far.r_idx[1, 64:68, 0].tolist() == [32] * 4 and (far.r_idx[1, 64:68, 1] < 0).all()
    assert _kinds_and_solutions(la, far, "anchor rows behind the pair") == CHAIN       # (WAVE6's verdict at this threshold as well)
    far.r_idx[1, 66] = (32, 31)
    a, h = _solver(la, far), _solver(la, far)
    _upload_dev(a, far); h.upload(far)
    for s in (a, h):
        s.solve_resident()
    assert a.last_kernel_kind() == h.last_kernel_kind() == GENERAL                       # not WAVE6: the second row on the pair was seen
    a.close(); h.close()
    assert _kinds_and_solutions(la, far, "a duplicated pair behind anchor rows") == CHAIN


def _refused(la, s, wb, admit=None):
    """upload_dev of wb is refused: (the error's text, admit as numpy)"""
    import torch
    dev = _dev(wb)
    torch.cuda.synchronize()
    with pytest.raises(la.LocalizationAmdError) as e:
        s.upload_dev(*dev, admit=admit)
    assert e.value.code == LOC_ERR_INVALID, e.value
    torch.cuda.synchronize()
    return str(e.value), None if admit is None else admit.cpu().numpy()


def test_the_only_bad_index_in_row_64_and_in_the_last_row(gpu):
    import localization_amd as la
    base = _step_window(la, True)
    s = _solver(la, base)
    for table, row, column, value, code in (("r_idx", 64, 0, 64, 2), ("r_idx", 129, 1, 64, 2), ("r_idx", 129, 1, -5, 2), ("p_idx", 64, None, 64, 4), ("p_idx", 69, None, -1, 4),
                                            ("s_idx", 64, 1, 64, 5), ("s_idx", 65, 0, -1, 5)):
        wb = base.copy()
        if column is None:
            getattr(wb, table)[1, row] = value
        else:
            getattr(wb, table)[1, row, column] = value
        text, _ = _refused(la, s, wb)
        assert WORDS[code] in text and "window 1" in text, (table, row, text)
    _upload_dev(s, base)                                       # the handle took none of them, and takes the window as it was
    s.close()


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------------------------------------------
def _rule(wb, bw_max, n_anchors):
    """tests/_window_structure_model.first_failed_check for every window of a WindowBatch"""
    b = types.SimpleNamespace(caps=tuple(wb.caps) + (bw_max,), counts=wb.counts, r_idx=wb.r_idx, p_idx=wb.p_idx, s_idx=wb.s_idx, n_anchors=n_anchors)
    return np.array([M.first_failed_check(b, i) for i in range(wb.B)], dtype=np.int32)


def _plant(la, base, i, code):
    wb = base.copy()
    nv = int(base.counts[i, 0])
    if code == 1:
        wb.counts[i, i % 4] = base.caps[i % 4] + 1 if i % 2 else -1
    elif code == 2:
        wb.r_idx[i, 0] = [(nv, 0), (1, -1 - len(P.ANCH)), (1, 1)][i % 3]
    elif code == 3:
        wb.r_idx[i, 0] = (0, 3) if i % 2 else (3, 0)
    elif code == 4:
        wb.p_idx[i, 0] = nv if i % 2 else -1
    elif code == 5:
        wb.s_idx[i, 0, :2] = [(nv, 0), (1, -1), (2, 2)][i % 3]
    else:
        wb.s_idx[i, 0, :2] = (0, 3) if i % 2 else (3, 0)
    return wb


@pytest.mark.parametrize("code", [1, 2, 3, 4, 5, 6])
def test_a_refused_batch_changes_nothing(gpu, code):
    import torch
    import localization_amd as la
    base = P.case_batch(la, "twist")[0]                        # eight windows of six poses: ranges, priors and EdgeSE3 rows; bw_max 2
    s = _solver(la, base, bw_max=2)
    _upload_dev(s, base); s.solve_resident()
    x0, t0 = _solved(la, s), s.download_batch()
    for i in (0, 3, base.B - 1):
        wb = _plant(la, _plant(la, base, base.B - 2, 7 - code), i, code) if i < base.B - 2 else _plant(la, base, i, code)
        want = _rule(wb, 2, len(P.ANCH))
        assert want[i] == code and np.flatnonzero(want)[0] == i
        admit = torch.full((wb.B,), -77, dtype=torch.int32, device="cuda")
        text, got = _refused(la, s, wb, admit)
        assert WORDS[code] in text and f"window {i})" in text, text
        assert got.tolist() == want.tolist()
        s.solve_resident()                                     # the previous resident batch: as it was, and it still solves
        _same_solution(_solved(la, s), x0, base.counts, (code, i))
        P.assert_same_tables(s.download_batch(), t0, (code, i))
    s.close()


def test_poisoned_rows_beyond_the_counts_change_nothing(gpu):
    import torch
    import localization_amd as la
    for name in ("twist", "imu"):
        base = P.case_batch(la, name, (2, 1, 1))[0]
        wb = base.copy()
        for i in range(wb.B):
            nv, nr, npr, ns = (int(x) for x in wb.counts[i])
            wb.poses[i, nv:] = np.nan; wb.r_idx[i, nr:] = (M.I32_MAX, M.I32_MIN); wb.p_idx[i, npr:] = M.I32_MIN; wb.s_idx[i, ns:] = (M.I32_MIN, M.I32_MAX, 7, 7)
            wb.r_val[i, nr:] = np.nan; wb.p_val[i, npr:] = np.inf; wb.s_val[i, ns:] = np.nan
        a, h = _solver(la, base), _solver(la, base)
        admit = torch.full((wb.B,), -77, dtype=torch.int32, device="cuda")
        _upload_dev(a, wb, admit); _upload_dev(h, base)
        assert admit.cpu().numpy().tolist() == [0] * wb.B
        for s in (a, h):
            s.solve_resident()
        assert a.last_kernel_kind() == h.last_kernel_kind() == (WAVE6S if name == "twist" else WAVE6)
        _same_solution(_solved(la, a), _solved(la, h), base.counts, name)
        a.close(); h.close()


def test_argument_refusals(gpu):
    import torch
    import localization_amd as la
    wb = P.case_batch(la, "twist")[0]
    s = _solver(la, wb)
    dev = _dev(wb)
    torch.cuda.synchronize()
    for change in (dict(n=0), dict(n=wb.B + 1), dict(counts=None), dict(poses=None), dict(r_val=None), dict(p_idx=None), dict(s_idx=None)):
        args = dict(zip(TABLES, dev), n=wb.B)
        args.update(change)
        with pytest.raises(la.LocalizationAmdError) as e:
            s.upload_dev(**args)
        assert e.value.code == LOC_ERR_INVALID
    with pytest.raises(la.LocalizationAmdError):                # nothing became resident
        s.solve_resident()
    s.close()


# ---- 4. the resident entries after it -----------------------------------------------------------------------------------------------------------------------
def _entries(la, s, wb, inputs):
    """every resident entry that reads the handle's state on a solved batch, as (name, bytes or error code) pairs; ends with a plain-drop slide"""
    import torch
    t = torch.device("cuda", 0)
    B, (nvm, nrm, npm, nsm) = wb.B, wb.caps
    z = lambda shape, dt=torch.float64: torch.zeros(shape, dtype=dt, device=t)
    out = []

    def call(name, f, *tensors):
        try:
            f()
            torch.cuda.synchronize()
            out.append((name, [x.cpu().numpy().tobytes() for x in tensors]))
        except la.LocalizationAmdError as e:
            out.append((name, e.code))
    cov, mask, status = z((B, nvm, 36)), z((B, nvm), torch.int32), z((B,), torch.int32)
    call("covariance", lambda: s.covariance_resident(cov, mask, status), cov, mask, status)
    jcov, jmask, jstatus, cross = z((B, nvm, 36)), z((B, nvm), torch.int32), z((B,), torch.int32), z((B, 2, 36))
    call("joint covariance", lambda: s.joint_covariance_resident(np.array([[0, 5], [4, 5]], dtype=np.int32), None, jcov, jmask, jstatus, cross), jcov, jmask, jstatus, cross)
    bad = z((B, 1, 36))                                        # a pair slot beyond the windows' poses: the pair check reads the counts
    call("joint covariance, a bad pair", lambda: s.joint_covariance_resident(np.array([[0, 6]], dtype=np.int32), None, jcov, jmask, jstatus, bad))
    chi = (z((B, nrm)), z((B, npm)), z((B, max(nsm, 1))), z((B,)), z((B,), torch.int32))
    call("edge chi2", lambda: s.edge_chi2_resident(*chi), *chi)
    flags, rt, opt, chi2, npub = z((B,), torch.int32), z((B, 7)), z((B, 7)), z((B,)), z((1,), torch.int32)
    call("publish", lambda: s.publish_resident(1e9, nvm, flags, rt, opt, chi2, npub), flags, rt, opt, chi2, npub)
    out.append(("tables", [getattr(s.download_batch(), name).tobytes() for name in TABLES]))
    anchors = np.ascontiguousarray(P.ANCH[:2])
    out.append(("set_anchors shrink", s.L.loc_window_set_anchors(s.h, 2, anchors.ctypes.data_as(C.POINTER(C.c_double)))))
    pose, ranges, priors, se3, drop = inputs
    d = lambda a, dt: torch.from_numpy(np.array(a, dtype=dt)).to(t)
    dev = (d(pose, np.float64), (d(ranges[0], np.int32), d(ranges[1], np.int32), d(ranges[2], np.float64)), (d(priors[0], np.int32), d(priors[1], np.float64)),
           (d(se3[0], np.int32), d(se3[1], np.int32), d(se3[2], np.float64)), None)
    st, ad = z((B,), torch.int32), z((B,), torch.int32)
    torch.cuda.synchronize()
    call("plain slide", lambda: s.slide_plain_resident_dev(*dev, out=(st, ad)), st, ad)
    out.append(("slid tables", [getattr(s.download_batch(), name).tobytes() for name in TABLES]))
    out.append(("set_anchors shrink after the slide", s.L.loc_window_set_anchors(s.h, 2, anchors.ctypes.data_as(C.POINTER(C.c_double)))))
    s.solve_resident()
    x = _solved(la, s)
    out.append(("solve after the slide", [x.poses.tobytes(), x.result.tobytes(), s.last_kernel_kind().encode()]))
    return out


@pytest.mark.parametrize("slide", [0, 1])
@pytest.mark.parametrize("name", ["imu", "twist"])
def test_the_resident_entries_after_it(gpu, name, slide):
    import localization_amd as la
    wb, streams, spec = P.case_batch(la, name)
    inputs = P.next_inputs(wb, streams, spec)
    a, h = _solver(la, wb, slide=slide), _solver(la, wb, slide=slide)
    _upload_dev(a, wb); h.upload(wb)
    got = []
    for s in (a, h):
        s.solve_resident()
        got.append(_entries(la, s, wb, inputs))
    for (what, x), (_, y) in zip(*got):
        assert x == y, (what, x if isinstance(x, int) else "bytes differ", y if isinstance(y, int) else "")
    codes = dict((what, x) for what, x in got[0] if isinstance(x, int))
    assert codes["set_anchors shrink"] == LOC_ERR_INVALID and codes["joint covariance, a bad pair"] == LOC_ERR_INVALID
    assert ("plain slide" in codes) == (slide == 0)            # without the option the slide is refused, by both handles alike
    a.close(); h.close()


@pytest.mark.parametrize("slide", [0, 1])
def test_the_anchor_table_may_shrink_to_the_largest_anchor_referenced_and_no_further(gpu, slide):
    """min_anchors comes from the admit pass's record (max_anchor_referenced on the host): exactly the largest anchor a used row names"""
    import localization_amd as la
    wb = P.case_batch(la, "imu")[0]
    wb.r_idx[:, :, 1][wb.r_idx[:, :, 1] == -4] = -3            # anchor 3 is not referenced any more ...
    wb.r_idx[7, int(wb.counts[7, 1]) - 1] = (int(wb.counts[7, 0]) - 1, -3)   # ... and anchor 2 by the last used row of the last window at least
    wb.r_idx[0, int(wb.counts[0, 1]):] = (0, -4)                # (rows beyond a count do not count)
    used = [int(-v) for i in range(wb.B) for v in wb.r_idx[i, :wb.counts[i, 1], 1].tolist() if v < 0]
    assert max(used) == 3
    a, h = _solver(la, wb, slide=slide), _solver(la, wb, slide=slide)
    _upload_dev(a, wb); h.upload(wb)
    dp = C.POINTER(C.c_double)
    shrink = lambda s, n: s.L.loc_window_set_anchors(s.h, n, np.ascontiguousarray(P.ANCH[:n]).ctypes.data_as(dp))
    for s in (a, h):
        assert [shrink(s, 2), shrink(s, 3), shrink(s, 2)] == [LOC_ERR_INVALID, 0, LOC_ERR_INVALID]
        s.solve_resident()
    _same_solution(_solved(la, a), _solved(la, h), wb.counts, "three anchors")
    a.close(); h.close()


@pytest.mark.parametrize("slide", [0, 1])
def test_a_push_of_messages_after_it(gpu, slide):
    import torch
    import localization_amd as la
    import test_gpu_message_rows as R
    name = "uwb_imu"
    wb = R._batch(la, name, nvs=(np.arange(24) % R.T) + 1, seed=21)
    msgs = R._messages(name, 0, wb, seed=21)
    mask = R.FAMILIES[name]["mask"]
    a, h = _solver(la, wb, slide=slide), _solver(la, wb, slide=slide)
    _upload_dev(a, wb); h.upload(wb)
    got = []
    for s in (a, h):
        R._config(s, R.M.Config(R.T)); s.solve_resident()
        dm = R._dev(R.M.masked(msgs, mask))
        verdict, status, admit = (torch.full((wb.B,), -77, dtype=torch.int32, device="cuda") for _ in range(3))
        torch.cuda.synchronize()
        try:
            s.push_messages_resident_dev(mask, dm, verdict=verdict, status=status, admit=admit)
            code = 0
        except la.LocalizationAmdError as e:
            code = e.code
        torch.cuda.synchronize()
        got.append([code] + [t.cpu().numpy().tobytes() for t in (verdict, status, admit)] + [getattr(s.download_batch(), n).tobytes() for n in TABLES])
    assert got[0] == got[1]
    assert (got[0][0] == 0) == (slide == 1)
    a.close(); h.close()


# ---- 5. stream order ---------------------------------------------------------------------------------------------------------------------------------------------
def test_the_tables_a_kernel_wrote_on_the_callers_stream(gpu):
    import torch
    import localization_amd as la
    wb = P.case_batch(la, "twist")[0]
    src = _dev(wb)
    dst = [torch.zeros_like(t) for t in src]                   # zeros: eight windows without poses, admitted as well
    busy = torch.randn(2048, 2048, device="cuda")
    a, h = _solver(la, wb), _solver(la, wb)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        for _ in range(20):                                    # the stream is busy for a while before the tables are written
            busy = busy @ busy * 1e-3
        for d, s_ in zip(dst, src):
            d.copy_(s_, non_blocking=True)
        a.upload_dev(*dst, stream=st)                          # queued right behind the writes: no synchronisation in between
    h.upload(wb)
    for s in (a, h):
        s.solve_resident()
    assert a.last_kernel_kind() == h.last_kernel_kind() == WAVE6S
    _same_solution(_solved(la, a), _solved(la, h), wb.counts, "stream order")
    P.assert_same_tables(a.download_batch(), wb, "stream order")
    a.close(); h.close()
