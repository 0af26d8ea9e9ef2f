"""A mixed forest batch uploaded from DEVICE arrays on the grouped kernel (loc_window_upload_dev under options "upload_dev_structures" +
"forest_groups" + "upload_dev_forest_groups"; window_groups_kernel.hip; DESIGN.md §2, "Upload from device arrays").  The yardstick is
loc_window_upload of the same arrays on a twin handle with "forest_groups" 1, BIT FOR BIT: the call groups and classifies, it computes no
number, so there is no tolerance anywhere (tests/test_gpu_forest_groups.py holds that twin to the oracle).  The grouping rule itself is held
to build_tree_groups without a GPU by tests/test_upload_dev_forest_groups_cpu.py.

The shapes of tests/test_gpu_forest_groups.py: 70 windows over 5 topologies (neighbouring waves of different groups, a T = 2 group, a
two-tree group, a random forest), more than one workgroup's four waves."""
import ctypes as C
import functools

import numpy as np
import pytest

import _forest_groups_cases as FC
import _slide_plain_ref as P
import test_gpu_upload_dev as U
from _forest_groups_cases import ANCH, CAPS

pytestmark = pytest.mark.gpu

B, G = 70, 5
OF = [b % G for b in range(B)]
GROUPS, GENERAL, TREE_WAVE, ARROW3 = "tree_wave_kernel<groups>", "window_lm_kernel", "tree_wave_kernel", "arrow3_lm_kernel"
COV_GROUPS = "forest_covariance_kernel<groups>"


def _handle(la, jac, dev, on=1, batch=B, **options):
    """dev: the handle that uploads from device arrays (the three options); else its twin, which takes the arrays through upload()"""
    s = la.WindowSolver(ANCH, batch, *CAPS, jacobian=jac, bw_max=CAPS[0] - 1, chain_threshold=1)
    s.set_option("forest_groups", 1)
    for k, v in options.items():
        s.set_option(k, v)
    if dev:
        s.set_option("upload_dev_structures", 1)
        s.set_option("upload_dev_forest_groups", on)                          # (a library without the option refuses the name)
    return s


def _pair(la, jac="analytic", **options):
    return _handle(la, jac, True, **options), _handle(la, jac, False, **options)


def _both(la, d, h, wb, kernel, what, groups=None):
    """wb through upload_dev on d and upload on h, a resident solve each: the same kernel, the same forest_groups(), the same bits"""
    U._upload_dev(d, wb); h.upload(wb)
    assert d.forest_groups() == h.forest_groups(), (what, d.forest_groups(), h.forest_groups())
    for s in (d, h):
        s.solve_resident()
    assert (d.last_kernel_kind(), h.last_kernel_kind()) == (kernel, kernel), (what, d.last_kernel_kind(), h.last_kernel_kind())
    assert d.forest_groups() == h.forest_groups()
    if groups is not None:
        assert d.forest_groups()[0] == groups and (d.forest_groups()[1] > 0) == (groups > 0), (what, d.forest_groups())
    U._same_solution(U._solved(la, d), U._solved(la, h), wb.counts, what)


@functools.lru_cache(maxsize=None)
def _mixed():
    import localization_amd as la
    return FC.mixed_batch(la, FC.five_topologies(), OF, 21)


@functools.lru_cache(maxsize=None)
def _twin(jac):
    """the twin's answer for the five-topology batch: (forest_groups(), the solved batch); shared, never modified"""
    import localization_amd as la
    h = _handle(la, jac, False)
    h.upload(_mixed()); h.solve_resident()
    assert h.last_kernel_kind() == GROUPS and h.forest_groups()[0] == G
    out = h.forest_groups(), U._solved(la, h)
    h.close()
    return out


# ---- 1. the feature ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jac", ["analytic", "numeric"])
def test_a_mixed_batch_from_device_arrays_takes_the_grouped_kernel(gpu, jac):
    import localization_amd as la
    wb = _mixed()
    groups, want = _twin(jac)
    d = _handle(la, jac, True)
    U._upload_dev(d, wb)
    assert d.forest_groups() == groups and groups[0] == G and groups[1] > 0
    d.solve_resident()
    assert d.last_kernel_kind() == GROUPS
    U._same_solution(U._solved(la, d), want, wb.counts, "the five topologies")
    d.close()


# ---- 2. default off ---------------------------------------------------------------------------------------------------------------------------------
def test_the_option_off_leaves_the_general_kernel(gpu):
    import localization_amd as la
    wb = _mixed()
    off = _handle(la, "analytic", True, on=0)
    never = _handle(la, "analytic", False, upload_dev_structures=1)           # the option never set
    for s in (off, never):
        U._upload_dev(s, wb); s.solve_resident()
        assert s.last_kernel_kind() == GENERAL and s.forest_groups() == (0, 0)
    U._same_solution(U._solved(la, off), U._solved(la, never), wb.counts, "option off")
    # ... and each of the other two options alone does not group either
    for options in (dict(upload_dev_structures=0), dict(forest_groups=0)):
        s = _handle(la, "analytic", True)
        for k, v in options.items():
            s.set_option(k, v)
        U._upload_dev(s, wb); s.solve_resident()
        assert s.last_kernel_kind() == GENERAL and s.forest_groups() == (0, 0), options
        U._same_solution(U._solved(la, s), U._solved(la, never), wb.counts, str(options))
        s.close()
    off.close(); never.close()


# ---- 3. hash collisions -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [0, 3])
def test_a_colliding_hash_changes_nothing(gpu, bits):
    """0 bits: every window collides with window 0; 3 bits: five keys in at most eight values, 70 windows — the answer is case 1's"""
    import localization_amd as la
    wb = _mixed()
    groups, want = _twin("analytic")
    d = _handle(la, "analytic", True, upload_dev_groups_hash_bits=bits)
    U._upload_dev(d, wb)
    assert d.forest_groups() == groups
    d.solve_resident()
    assert d.last_kernel_kind() == GROUPS
    U._same_solution(U._solved(la, d), want, wb.counts, f"{bits} hash bits")
    for bad in (-1, 65):
        with pytest.raises(la.LocalizationAmdError):
            d.set_option("upload_dev_groups_hash_bits", bad)
    d.close()


# ---- 4. orders of appearance ------------------------------------------------------------------------------------------------------------------------
def test_orders_of_appearance_a_topology_per_window_and_one_topology(gpu):
    import localization_amd as la
    topos = FC.five_topologies()
    d, h = _pair(la)
    back = FC.mixed_batch(la, topos, [4 - b % 5 for b in range(B)], 22)                       # the groups do not first appear in the topologies' order
    _both(la, d, h, back, GROUPS, "4 - b % 5", groups=5)
    last = FC.mixed_batch(la, topos, [4 if b == B - 1 else b % 4 for b in range(B)], 23)      # window B - 1 opens a group
    _both(la, d, h, last, GROUPS, "the last window opens a group", groups=5)
    own = [FC.star(2 + b, 5, n_anchor=2, lever=True) for b in range(63)] + [FC.star(10 + b, 2, n_anchor=2, lever=True) for b in range(B - 63)]
    _both(la, d, h, FC.mixed_batch(la, own, list(range(B)), 17), GROUPS, "G = B", groups=B)
    one = FC.mixed_batch(la, [FC.star(40, 6, first=2)], [0] * B, 18)                          # one topology, other anchors per window: still grouped
    assert all((one.r_idx[b, :40, 1] != one.r_idx[b + 1, :40, 1]).all() for b in range(B - 1))
    _both(la, d, h, one, GROUPS, "G = 1", groups=1)
    same = FC.mixed_batch(la, topos, [2] * B, 14, vary=False)                                 # a true one-topology batch keeps its kernel
    _both(la, d, h, same, TREE_WAVE, "one topology", groups=0)
    assert d.forest_groups() == (0, 0)
    _both(la, d, h, back, GROUPS, "4 - b % 5 again", groups=5)
    d.close(); h.close()


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------------------
def _refusal(la, name):
    """(batch, options, prepare)"""
    topos = FC.five_topologies()
    wb, options, prepare = _mixed().copy(), {}, None
    if name == "a window with one pose":
        wb = FC.mixed_batch(la, topos + [FC.star(1, 1, n_anchor=3)], [5 if b == 37 else b % 5 for b in range(B)], 24)
        assert wb.counts[37, 0] == 1
    elif name == "a cycle in one group":
        assert OF[7] == 2
        wb.add_range(7, 20, 33, 1.0, 10.0)                                    # window 7 (T = 40): a loop closure between two poses of one tree
    elif name == "two EdgeSE3 on one pair":
        assert OF[10] == 0
        vi, vj = (int(v) for v in wb.s_idx[10, 5, :2])
        wb.add_se3(10, vi, vj, np.zeros(3), np.eye(3), np.eye(6) * 2e3, True)
    elif name == "below tree_min_batch":
        options = dict(chain_min_batch=B + 1)
    elif name == "tree = 0":
        options = dict(tree=0)
    elif name == "tree = 2":
        options = dict(tree=2)
    else:
        assert name == "endpoint-1 lever arms"
        off1 = np.zeros((B, CAPS[1], 3)); off1[:, :, 0] = 0.05
        wb.r_off1 = off1                                                      # (upload() hands the batch's table to its handle; upload_dev leaves the handle's as it is)
        def prepare(s):
            assert s.L.loc_window_set_endpoint1_offsets(s.h, B, off1.ctypes.data_as(C.POINTER(C.c_double))) == 0
    return wb, options, prepare


REFUSALS = ["a window with one pose", "a cycle in one group", "two EdgeSE3 on one pair", "below tree_min_batch", "tree = 0", "tree = 2", "endpoint-1 lever arms"]


@pytest.mark.parametrize("name", REFUSALS)
def test_a_refusal_is_the_hosts(gpu, name):
    import localization_amd as la
    wb, options, prepare = _refusal(la, name)
    d, h = _pair(la, **options)
    if prepare:
        prepare(d)
    _both(la, d, h, wb, GENERAL, name, groups=0)
    d.close(); h.close()


# ---- 6. covariances ---------------------------------------------------------------------------------------------------------------------------------
def test_the_first_covariance_call_walks_the_uploaded_block(gpu):
    import torch
    import localization_amd as la
    wb = _mixed()
    d, h = _pair(la, "numeric", forest_groups_covariance=1)
    _both(la, d, h, wb, GROUPS, "the five topologies", groups=G)
    fresh = lambda npm=None: [torch.full((B, CAPS[0], 6, 6), 7.0, dtype=torch.float64, device=gpu), torch.full((B, CAPS[0]), 7, dtype=torch.int32, device=gpu),
                              torch.full((B,), 7, dtype=torch.int32, device=gpu)] + ([] if npm is None else [torch.full((B, npm, 6, 6), 7.0, dtype=torch.float64, device=gpu)])
    host = lambda ts: [t.cpu().numpy() for t in ts]
    same = lambda x, y: all(np.array_equal(p, q, equal_nan=True) for p, q in zip(x, y, strict=True))
    out = {}
    for s in (d, h):
        assert s.last_covariance_kind() == "none"
        plain = fresh()
        s.covariance_resident(*plain)                                         # the FIRST call: the block of the upload, no copy-back, no block of its own
        torch.cuda.synchronize()
        assert s.last_covariance_kind() == COV_GROUPS
        pairs = np.tile(np.array([[0, 1], [1, 0], [1, 1]], dtype=np.int32), (B, 1, 1))
        counts = np.array([3 - b % 3 for b in range(B)], dtype=np.int32)
        joint = fresh(3)
        s.joint_covariance_resident(pairs, counts, *joint)
        torch.cuda.synchronize()
        assert s.last_covariance_kind() == COV_GROUPS
        out[s] = host(plain), host(joint)
    assert same(out[d][0], out[h][0]) and same(out[d][1], out[h][1])
    ok = out[d][0][2] == 0                                                    # (the pass computed something: finite blocks wherever it reports success)
    assert ok.any() and np.isfinite(out[d][0][0][ok]).all() and np.nanmax(np.abs(out[d][1][3])) > 0
    d.close(); h.close()


# ---- 7. a batch refused at admission ----------------------------------------------------------------------------------------------------------------
def test_a_batch_refused_at_admission_leaves_the_grouped_batch(gpu):
    import localization_amd as la
    wb = _mixed()
    groups, want = _twin("analytic")
    d = _handle(la, "analytic", True)
    U._upload_dev(d, wb); d.solve_resident()
    assert d.last_kernel_kind() == GROUPS and d.forest_groups() == groups
    bad = FC.mixed_batch(la, FC.five_topologies()[:3], [(b * 2) % 3 for b in range(40)], 25)  # other groups, other tables — and window 6 names a pose beyond its count
    bad.r_idx[6, 5, 0] = int(bad.counts[6, 0])
    text, _ = U._refused(la, d, bad)
    assert "range edge vertex index" in text and "window 6" in text
    assert d.forest_groups() == groups
    d.solve_resident()
    assert d.last_kernel_kind() == GROUPS and d.forest_groups() == groups
    U._same_solution(U._solved(la, d), want, wb.counts, "the old batch after the refusal")
    d.close()


# ---- 8. re-upload on one handle ---------------------------------------------------------------------------------------------------------------------
def test_grouped_then_an_arrowhead_then_grouped_on_one_handle(gpu):
    import localization_amd as la
    arrow = la.WindowBatch(12, *CAPS)                                         # five chain and two border poses, translation-only
    rng = np.random.default_rng(19)
    for i in range(arrow.B):
        xs = np.cumsum(rng.normal(0.0, 0.1, (7, 3)), axis=0) + (0.5, 0.2, 1.0)
        for k in range(7):
            arrow.add_pose(i, xs[k] + rng.normal(0.0, 0.01, 3))
        for v0, v1 in [(3, 6), (0, 5), (1, 0), (2, 1), (6, 5), (2, 3), (4, 3), (0, 6)] + [(k, -1 - k % 4) for k in range(7)]:
            arrow.add_range(i, v0, v1, float(np.linalg.norm(xs[v0] - (ANCH[-1 - v1] if v1 < 0 else xs[v1])) + rng.normal(0.0, 0.02)), P.RANGE_INFO)
    other = FC.mixed_batch(la, FC.five_topologies()[:3], [(b * 2) % 3 for b in range(40)], 26)
    d, h = _pair(la, arrow3=1)
    for wb, kernel, groups in ((_mixed(), GROUPS, 5), (arrow, ARROW3, 0), (other, GROUPS, 3), (arrow, ARROW3, 0), (_mixed(), GROUPS, 5)):
        _both(la, d, h, wb, kernel, kernel, groups=groups)
    d.close(); h.close()
