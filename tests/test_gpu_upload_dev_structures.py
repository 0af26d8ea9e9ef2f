"""Forest and arrowhead verdicts of a batch uploaded from DEVICE arrays (loc_window_upload_dev under option "upload_dev_structures";
window_structure_kernel.hip; DESIGN.md §2, "Upload from device arrays").  The yardstick is loc_window_upload of the same arrays on a second
handle with the same options, BIT FOR BIT: the call classifies and packs, it computes no number, so there is no tolerance anywhere.  The
arrowhead rule itself, window by window, is held to build_arrow_aux without a GPU by tests/test_arrow_pack_cpu.py.

Batches of 6 to 12 windows: more than one workgroup's four waves, so partial records are merged."""
import ctypes as C

import numpy as np
import pytest

import _slide_plain_ref as P
import _window_structure_model as M
import test_gpu_upload_dev as U

pytestmark = pytest.mark.gpu

GENERAL, ARROW3, TREE_WAVE, TREE_LANE = "window_lm_kernel", "arrow3_lm_kernel", "tree_wave_kernel", "tree_lm_kernel"
LOC_ERR_UNSUPPORTED = -5
INFO3 = (4.0, 4.0, 4.0, 0.0, 0.0, 0.0)


def _pair(la, wb, jac="analytic", anchors=None, bw_max=-1, **options):
    """(the handle that uploads from device arrays with the option on, the handle that uploads from the host), the same options otherwise"""
    out = []
    for on in (1, 0):
        s = la.WindowSolver(P.ANCH if anchors is None else anchors, wb.B, *wb.caps, jacobian=jac, bw_max=bw_max)
        for k, v in options.items():
            s.set_option(k, v)
        s.set_option("upload_dev_structures", on)
        out.append(s)
    return out


def _both(la, wb, jac="analytic", anchors=None, prepare=None, bw_max=-1, **options):
    """upload_dev (option on) and upload of wb, a resident solve each: (a, h)"""
    a, h = _pair(la, wb, jac, anchors, bw_max, **options)
    for s in (a, h):
        if prepare:
            prepare(s)
    U._upload_dev(a, wb); h.upload(wb)
    for s in (a, h):
        s.solve_resident()
    return a, h


def _same_kernel_and_bits(la, a, h, wb, kernel, what):
    assert (a.last_kernel_kind(), h.last_kernel_kind()) == (kernel, kernel), (what, a.last_kernel_kind(), h.last_kernel_kind())
    U._same_solution(U._solved(la, a), U._solved(la, h), wb.counts, what)


def _poison(wb):
    """garbage beyond every count"""
    for i in range(wb.B):
        nv, nr, npr, ns = (int(x) for x in wb.counts[i])
        wb.poses[i, nv:] = np.nan; wb.r_idx[i, nr:] = (M.I32_MAX, M.I32_MIN); wb.r_val[i, nr:] = np.nan
        wb.p_idx[i, npr:] = M.I32_MIN; wb.p_val[i, npr:] = np.inf; wb.s_idx[i, ns:] = (M.I32_MIN, M.I32_MAX, 7, 7); wb.s_val[i, ns:] = np.nan
    return wb


# ---- arrowhead batches ----------------------------------------------------------------------------------------------------------------------------------
def _arrow_window(wb, i, rng, n0, nb0, anchors=P.ANCH, shuffle=True, rich=True):
    """a translation-only window of n0 chain poses and nb0 border poses: a range per consecutive chain pair (either direction), (0, n0) and
    further chain-border ranges, border-border ranges, two anchor ranges per pose; the rows in a random order (NOT the rows' order);
    rich: two priors on a chain pose, one on a border pose, one on every separator"""
    nv = n0 + nb0
    xs = np.cumsum(rng.normal(0.0, 0.08, (nv, 3)), axis=0) + (0.5, 0.2, 1.0)
    xs[n0:] = rng.uniform(-2.0, 2.0, (nb0, 3)) + (0.0, 0.0, 1.0)
    for k in range(nv):
        wb.add_pose(i, xs[k] + rng.normal(0.0, 0.01, 3))
    edges = [(k - 1, k) if rng.random() < 0.5 else (k, k - 1) for k in range(1, n0)] + [(0, n0)]
    for a in range(nb0):
        edges += [(k, n0 + a) if rng.random() < 0.6 else (n0 + a, k) for k in range(n0) if rng.random() < 0.3 and (k, a) != (0, 0)]
        edges += [(n0 + a, n0 + c) if rng.random() < 0.5 else (n0 + c, n0 + a) for c in range(a) if rng.random() < 0.5]
    edges += [(k, -1 - int(rng.integers(4))) for k in range(nv) for _ in range(2)]
    for k in (rng.permutation(len(edges)) if shuffle else range(len(edges))):
        v0, v1 = edges[k]
        x1 = anchors[-1 - v1] if v1 < 0 else xs[v1]
        wb.add_range(i, v0, v1, float(np.linalg.norm(xs[v0] - x1) + rng.normal(0.0, 0.02)), P.RANGE_INFO)
    if rich:
        nseg = M.arrow_nseg(n0)
        for v in [1, n0, 1] + [k * n0 // nseg for k in range(1, nseg)]:
            wb.add_prior(i, v, xs[v] + rng.normal(0.0, 0.05, 3), np.eye(3), info_diag=INFO3)
    assert M.arrow_border(wb_view(wb), i) == nb0


class wb_view:
    """a WindowBatch as tests/_window_structure_model.py reads batches"""
    def __init__(self, wb):
        self.counts, self.r_idx = wb.counts, wb.r_idx


SHAPES = [(3, 1), (25, 2), (46, 5), (63, 12), (74, 1), (98, 12), (105, 5), (26, 1)]   # nv = 4, 27, 51, 75, 75, 110, 110, 27: one .. four segments


def _arrow_batch(la, seed=3):
    rng = np.random.default_rng(seed)
    wb = la.WindowBatch(len(SHAPES), 110, 900, 12, 0)
    for i, (n0, nb0) in enumerate(SHAPES):
        _arrow_window(wb, i, rng, n0, nb0)
    assert [M.arrow_nseg(n0) for n0, _ in SHAPES] == [1, 1, 1, 2, 3, 4, 4, 1] and wb.counts[:, 0].tolist() == [4, 27, 51, 75, 75, 110, 110, 27]
    return _poison(wb)


def _resident_entries(la, s, wb):
    """what the resident entries answer on a solved batch: (name, bytes or error code)"""
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
    call("joint covariance", lambda: s.joint_covariance_resident(np.array([[0, 1], [3, 2]], dtype=np.int32), None, jcov, jmask, jstatus, cross), jcov, jmask, jstatus, cross)
    chi = (z((B, nrm)), z((B, max(npm, 1))), z((B, max(nsm, 1))), z((B,)), z((B,), torch.int32))
    call("edge chi2", lambda: s.edge_chi2_resident(*chi), *chi)
    P.assert_same_tables(s.download_batch(), wb, "download_tables against the inputs")
    removed, n_removed = z((B, nrm), torch.int32), z((B,), torch.int32)
    call("prune", lambda: s.prune_resident(2.0, 3, removed, n_removed), removed, n_removed)
    return out


def _assert_same_entries(got_a, got_h):
    for (what, x), (_, y) in zip(got_a, got_h):
        assert x == y, (what, x if isinstance(x, int) else "bytes differ", y if isinstance(y, int) else "")
    return dict(got_a)


@pytest.mark.parametrize("jac", ["analytic", "numeric"])
def test_a_ragged_arrowhead_batch(gpu, jac):
    import localization_amd as la
    wb = _arrow_batch(la)
    a, h = _both(la, wb, jac)
    _same_kernel_and_bits(la, a, h, wb, ARROW3, "the ragged arrowhead batch")
    got = _assert_same_entries(_resident_entries(la, a, wb), _resident_entries(la, h, wb))
    assert not isinstance(got["covariance"], int) and not isinstance(got["joint covariance"], int) and not isinstance(got["edge chi2"], int)
    assert got["prune"] == LOC_ERR_UNSUPPORTED                      # an ARROW3 batch: the records were packed at upload
    o = la.WindowSolver(P.ANCH, wb.B, *wb.caps, jacobian=jac)     # the option off: today's upload_dev
    U._upload_dev(o, wb); o.solve_resident()
    assert o.last_kernel_kind() == GENERAL
    for s in (a, h, o):
        s.close()


def _small_arrow(la, n_anchors=4, np_max=20, nv_max=70, extra=0):
    """six plain arrowhead windows of 20 chain and 2 border poses, ordered rows, no priors; the anchor table"""
    anchors = P.ANCH if n_anchors == 4 else np.random.default_rng(1).uniform(-3.0, 3.0, (n_anchors, 3))
    rng = np.random.default_rng(11)
    wb = la.WindowBatch(6, nv_max, 160 + extra, np_max, 0)
    for i in range(6):
        _arrow_window(wb, i, rng, 20, 2, anchors=anchors, shuffle=False, rich=False)
    return wb, anchors


def _add(wb, i, v0, v1, anchors=P.ANCH):
    x = wb.poses[i, :, 9:]
    wb.add_range(i, v0, v1, float(np.linalg.norm(x[v0] - (anchors[-1 - v1] if v1 < 0 else x[v1]))), P.RANGE_INFO)


def _refusal(la, name):
    """(batch, anchors, options): window 5 (the second workgroup's) carries the refusal"""
    wb, anchors = _small_arrow(la)
    options = {}
    if name == "nb0 = 13":
        wb.counts[5] = 0
        _arrow_window(wb, 5, np.random.default_rng(13), 6, 13, shuffle=False, rich=False)
    elif name == "no border: a window of two poses":          # (nv - nb0 < 2 itself needs a non-consecutive range that ends at slot 1: there is none)
        wb.counts[5] = 0
        for k in range(2):
            wb.add_pose(5, (0.3 * k, 0.0, 1.0))
        _add(wb, 5, 0, 1); _add(wb, 5, 0, -1); _add(wb, 5, 1, -2)
    elif name == "a second range on a consecutive chain pair":
        _add(wb, 5, 7, 6)
    elif name == "an anchor code of 256":
        wb, anchors = _small_arrow(la, n_anchors=300)
        _add(wb, 5, 3, -257, anchors)
    elif name == "a row with 65 ranges":
        while _records_of_row(wb, 5, 1, 20) < 65:              # row 1: its chain link, two anchor ranges, its ranges to the border, and these
            _add(wb, 5, 1, -1)
    elif name == "a pose with 17 priors":
        for _ in range(17):
            wb.add_prior(5, 21, wb.poses[5, 21, 9:], np.eye(3), info_diag=INFO3)
    elif name == "nv_max fails arrow3_fits":
        wb = la.WindowBatch(6, 529, 800, 4, 0)
        rng = np.random.default_rng(17)
        for i in range(6):
            _arrow_window(wb, i, rng, *((96, 12) if i == 5 else (20, 2)), shuffle=False, rich=False)
        assert M.arrow3_lds_bytes(529, 15) > M.ARROW_LDS_LIMIT >= M.arrow3_lds_bytes(529, 14)
    elif name == "arrow3 = 0":
        options = dict(arrow3=0)
    else:
        assert name == "a rotation in one pose"
        wb.poses[5, 4, :9] = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]).reshape(9)
    return wb, anchors, options


def _records_of_row(wb, i, row_pose, n0):
    """the range rows the chain pose row_pose owns: its anchor ranges, its link to the previous pose, its ranges to border poses"""
    own = 0
    for v0, v1 in wb.r_idx[i, :wb.counts[i, 1]].tolist():
        if v1 < 0:
            own += v0 == row_pose
        elif max(v0, v1) >= n0:
            own += min(v0, v1) == row_pose
        else:
            own += max(v0, v1) == row_pose
    return own


REFUSALS = ["nb0 = 13", "no border: a window of two poses", "a second range on a consecutive chain pair", "an anchor code of 256", "a row with 65 ranges",
            "a pose with 17 priors", "nv_max fails arrow3_fits", "arrow3 = 0", "a rotation in one pose"]


@pytest.mark.parametrize("name", REFUSALS)
def test_an_arrowhead_refusal_is_the_hosts(gpu, name):
    import localization_amd as la
    wb, anchors, options = _refusal(la, name)
    if name == "a row with 65 ranges":
        assert _records_of_row(wb, 5, 1, 20) == 65 and _records_of_row(wb, 4, 1, 20) <= 64
    if name == "nv_max fails arrow3_fits":
        options["bw_max"] = 108                                  # (the general kernel's envelope: no range spans more)
    if name not in ("arrow3 = 0", "a rotation in one pose"):       # the batch is refused for THIS reason: without window 5's change it is taken
        base, base_anchors = _small_arrow(la, n_anchors=len(anchors), nv_max=wb.caps[0] if wb.caps[0] != 529 else 70)
        c = la.WindowSolver(base_anchors, base.B, *base.caps, jacobian="analytic")
        c.upload(base); c.solve_resident()
        assert c.last_kernel_kind() == ARROW3
        c.close()
    a, h = _both(la, wb, anchors=anchors, **options)
    _same_kernel_and_bits(la, a, h, wb, GENERAL, name)
    a.close(); h.close()


def test_every_arrowhead_refusal_has_its_taken_twin(gpu):
    """63 more ranges on a row (64 records) and 16 priors on a pose are taken, by both uploads"""
    import localization_amd as la
    wb, _ = _small_arrow(la)
    while _records_of_row(wb, 5, 1, 20) < 64:
        _add(wb, 5, 1, -1)
    for _ in range(16):
        wb.add_prior(5, 21, wb.poses[5, 21, 9:], np.eye(3), info_diag=INFO3)
    assert _records_of_row(wb, 5, 1, 20) == 64
    a, h = _both(la, wb)
    _same_kernel_and_bits(la, a, h, wb, ARROW3, "64 records, 16 priors")
    a.close(); h.close()


# ---- forest batches -------------------------------------------------------------------------------------------------------------------------------------
def _forest(la, every=4, B=8):
    import test_gpu_tree_parity as F
    assert F.ANCH.tobytes() == P.ANCH.tobytes()
    return F._forest_batch(la, np.random.default_rng(77), B, 8, every, False)


def _forest_variant(la, name):
    """(batch, options, prepare, kernel)"""
    wb, options, prepare, kernel = _forest(la), dict(chain_min_batch=1), None, TREE_WAVE
    if name == "tree = 2":
        options["tree"] = 2; kernel = TREE_LANE
    elif name == "one used index differs in the last window":
        wb.r_idx[7, int(wb.counts[7, 1]) - 1, 1] = -2 if wb.r_idx[7, int(wb.counts[7, 1]) - 1, 1] != -2 else -3
        kernel = GENERAL
    elif name == "indices differ beyond the counts":
        _poison(wb)
        wb.r_idx[3, int(wb.counts[3, 1]):] = (1, 2); wb.s_idx[6, int(wb.counts[6, 3]):] = (0, 7, 1, 0); wb.p_idx[2, int(wb.counts[2, 2]):] = 5
    elif name == "one count differs":
        wb.counts[6, 1] -= 1; kernel = GENERAL
    elif name == "a cycle in every window":
        for i in range(wb.B):
            wb.add_range(i, 1, 2, 0.3, P.SMOOTH_INFO)           # 0 - 1, 0 - 2 are EdgeSE3 rows
        kernel = GENERAL
    elif name == "tree = 0":
        options["tree"] = 0; kernel = GENERAL
    elif name == "endpoint-1 lever arms":
        off1 = np.zeros((wb.B, wb.caps[1], 3)); off1[:, :, 0] = 0.05
        wb.r_off1 = off1                                        # (upload() hands the batch's table to its handle; upload_dev leaves the handle's as it is)
        def prepare(s):
            assert s.L.loc_window_set_endpoint1_offsets(s.h, wb.B, off1.ctypes.data_as(C.POINTER(C.c_double))) == 0
        kernel = GENERAL
    else:
        assert name == "as it is"
    return wb, options, prepare, kernel


FORESTS = ["as it is", "tree = 2", "one used index differs in the last window", "indices differ beyond the counts", "one count differs", "a cycle in every window",
           "tree = 0", "endpoint-1 lever arms"]


@pytest.mark.parametrize("name", FORESTS)
def test_a_forest_verdict_is_the_hosts(gpu, name):
    import localization_amd as la
    wb, options, prepare, kernel = _forest_variant(la, name)
    a, h = _both(la, wb, prepare=prepare, **options)
    _same_kernel_and_bits(la, a, h, wb, kernel, name)
    a.close(); h.close()


@pytest.mark.parametrize("jac", ["analytic", "numeric"])
def test_a_forest_batch_and_its_resident_entries(gpu, jac):
    import localization_amd as la
    wb = _forest(la)
    a, h = _both(la, wb, jac, chain_min_batch=1)
    _same_kernel_and_bits(la, a, h, wb, TREE_WAVE, "the key-frame stars")
    got = _assert_same_entries(_resident_entries(la, a, wb), _resident_entries(la, h, wb))
    assert not any(isinstance(v, int) for v in got.values()), got
    a.close(); h.close()


def test_a_batch_below_the_forest_threshold_and_the_threshold_lowered_afterwards(gpu):
    import localization_amd as la
    wb = _forest(la)
    a, h = _both(la, wb)                                           # default options: eight windows are below tree_min_batch
    _same_kernel_and_bits(la, a, h, wb, GENERAL, "below the threshold")
    for s in (a, h):
        s.L.loc_window_set_chain_threshold(s.h, 1)
        s.solve_resident()
    assert a.last_kernel_kind() == h.last_kernel_kind()           # the verdict was taken at upload, on both
    U._same_solution(U._solved(la, a), U._solved(la, h), wb.counts, "threshold 1 afterwards")
    a.close(); h.close()


def test_a_forest_that_is_a_chain_in_another_edge_order(gpu):
    """every pose a key: EdgeSE3 rows k - 1 -> k; two rows swapped in every window make it an unordered chain — a forest for the solve, the
    chain pass's for the covariances, which the first covariance call finds out on both handles"""
    import localization_amd as la
    wb = _forest(la, every=1)
    for t in (wb.s_idx, wb.s_val):
        t[:, [2, 5]] = t[:, [5, 2]]
    a, h = _both(la, wb, chain_min_batch=1)
    _same_kernel_and_bits(la, a, h, wb, TREE_WAVE, "the unordered chain")
    got = _assert_same_entries(_resident_entries(la, a, wb), _resident_entries(la, h, wb))
    assert not isinstance(got["covariance"], int)
    a.close(); h.close()


# ---- state ------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_chain_batch_is_handled_as_without_the_option(gpu):
    import localization_amd as la
    for name, kernel in (("imu", U.WAVE6), ("twist", U.WAVE6S)):
        wb = P.case_batch(la, name)[0]
        on, off = _pair(la, wb)
        for s in (on, off):
            U._upload_dev(s, wb); s.solve_resident()
        _same_kernel_and_bits(la, on, off, wb, kernel, name)
        P.assert_same_tables(on.download_batch(), off.download_batch(), name)
        on.close(); off.close()


def test_a_refused_batch_leaves_the_resident_arrowhead_batch(gpu):
    import localization_amd as la
    wb = _arrow_batch(la)
    a, h = _both(la, wb)
    _same_kernel_and_bits(la, a, h, wb, ARROW3, "before")
    x0 = U._solved(la, a)
    bad = _arrow_batch(la, seed=4).copy()               # other records, other sizes — and window 6 names a pose beyond its count
    bad.r_idx[6, 5, 0] = int(bad.counts[6, 0])
    text, _ = U._refused(la, a, bad)
    assert "range edge vertex index" in text and "window 6" in text
    a.solve_resident()
    assert a.last_kernel_kind() == ARROW3
    U._same_solution(U._solved(la, a), x0, wb.counts, "the old batch after the refusal")
    a.close(); h.close()


def test_a_forest_after_an_arrowhead_on_one_handle_and_back(gpu):
    import localization_amd as la
    forest = _forest(la)
    arrow = la.WindowBatch(forest.B, *forest.caps)                 # five chain and two border poses under the forest batch's capacities
    rng = np.random.default_rng(19)
    for i in range(arrow.B):
        xs = np.cumsum(rng.normal(0.0, 0.1, (7, 3)), axis=0) + (0.5, 0.2, 1.0)
        for k in range(7):
            arrow.add_pose(i, xs[k] + rng.normal(0.0, 0.01, 3))
        for v0, v1 in [(3, 6), (0, 5), (1, 0), (2, 1), (6, 5), (2, 3), (4, 3), (0, 6)] + [(k, -1 - k % 4) for k in range(7)]:
            arrow.add_range(i, v0, v1, float(np.linalg.norm(xs[v0] - (P.ANCH[-1 - v1] if v1 < 0 else xs[v1])) + rng.normal(0.0, 0.02)), P.RANGE_INFO)
        arrow.add_prior(i, 2, xs[2], np.eye(3), info_diag=INFO3)
    a, h = _pair(la, forest, arrow3=1, chain_min_batch=1)
    for wb, kernel in ((arrow, ARROW3), (forest, TREE_WAVE), (arrow, ARROW3), (forest, TREE_WAVE)):
        U._upload_dev(a, wb); h.upload(wb)
        for s in (a, h):
            s.solve_resident()
        _same_kernel_and_bits(la, a, h, wb, kernel, kernel)
        _assert_same_entries(_resident_entries(la, a, wb), _resident_entries(la, h, wb))
    a.close(); h.close()
