"""Test helper: windows of every structure window_lm_kernel's structure analysis tells apart — loops, grids, cliques, forests, several
components, arrowheads — as plain pair lists, the batches tests/test_gpu_window_structures.py solves, and their oracle solves.

A window built by fill_graph is regular by the reference alone: every pose is ranged to all four anchors (6-DoF: with a lever arm and an
IMU rotation prior), so nothing is gauge-free whatever the pose-to-pose edges are.  Only the STRUCTURE varies between the families: the
trajectories, noise levels and weights are those of tests/_general_cov_inputs.py."""
import functools

import numpy as np
from scipy.spatial.transform import Rotation

from _general_cov_inputs import ANCH, IMU_INFO, LEVER, _anchor_ranges, _se3, _trajectory, fill_arrowhead6, window_pairs


# ---- pair builders: lists of (slot, slot) ---------------------------------------------------------------------------------------------
def chain(n):
    return [(k, k + 1) for k in range(n - 1)]


def ring(n):
    return [(k, (k + 1) % n) for k in range(n)]


def grid(r, c):
    return [(a * c + b, a * c + b + 1) for a in range(r) for b in range(c - 1)] + [(a * c + b, (a + 1) * c + b) for a in range(r - 1) for b in range(c)]


def random_tree(rng, n):
    return [(int(rng.integers(0, k)), k) for k in range(1, n)]


def chain_with_clique(n, m):
    """a chain of n poses whose last m poses are a clique"""
    return chain(n) + [(a, b) for a in range(n - m, n) for b in range(a + 2, n)]


def clique(n):
    return [(a, b) for a in range(n) for b in range(a + 1, n)]


def components(n):
    """a chain of n // 2 poses and a ring of the rest, no edge between them"""
    h = n // 2
    return chain(h) + [(h + u, h + v) for u, v in ring(n - h)]


def ladder(n):
    """two rails of n poses (even / odd slots) and n rungs"""
    return [(2 * k, 2 * k + 1) for k in range(n)] + [(2 * k, 2 * k + 2) for k in range(n - 1)] + [(2 * k + 1, 2 * k + 3) for k in range(n - 1)]


def banded_with_long_links(n, spans):
    """a chain with, per (span, every, first), a link k -- k + span from every `every`-th pose on"""
    return chain(n) + [(k, k + span) for span, every, first in spans for k in range(first, n - span, every)]


def arrowhead(T, A):
    """a chain of T poses, each joined to all A border poses (slots T .. T + A - 1)"""
    return chain(T) + [(k, T + a) for k in range(T) for a in range(A)]


def arrowhead_with_pendant(T, A):
    """arrowhead(T, A) and one pendant pose (slot T + A) on the first border pose"""
    return arrowhead(T, A) + [(T, T + A)]


def pair_count(pairs):
    return 1 + max(max(p) for p in pairs)


# ---- windows --------------------------------------------------------------------------------------------------------------------------
def fill_graph(wb, i, rng, T, pairs, six_dof, doubled=()):
    """every pose ranged to all four anchors; six_dof: a lever arm and an IMU rotation prior per pose.  Pair n of `pairs`: six_dof and n % 3 == 0:
    a robust full-information EdgeSE3 (every other one stored flipped); else a measured range.  Pairs numbered in `doubled` get a second, weaker
    range (a shared pair: result[6])."""
    tt, tR, et, eR = _trajectory(rng, T, six_dof)
    off = LEVER if six_dof else np.zeros(3)
    for k in range(T): wb.add_pose(i, et[k], eR[k])
    for k in range(T):
        _anchor_ranges(wb, i, k, tt[k], tR[k], off, rng)
        if six_dof:
            wb.add_prior(i, k, et[k], (tR[k] * Rotation.from_rotvec(rng.normal(0, 2e-3, 3))).as_matrix(), IMU_INFO)
    for n, (u, v) in enumerate(pairs):
        if six_dof and n % 3 == 0:
            _se3(wb, i, rng, tt, tR, u, v, u, v, flip=n % 2 == 1, scale=1e3)
        else:
            wb.add_range(i, u, v, float(np.linalg.norm(tt[u] - tt[v]) + rng.normal(0, 0.01)), 1 / 0.1 ** 2)
    for n in doubled:
        u, v = pairs[n]
        wb.add_range(i, v, u, float(np.linalg.norm(tt[u] - tt[v])), 1 / 0.2 ** 2)


def relabel(wb, i, perm):
    """Window i of wb, in place, with pose slot k moved to perm[k]: poses, r_idx, p_idx and s_idx rewritten, every edge in its place."""
    nv, nr, npr, ns = (int(x) for x in wb.counts[i])
    perm = np.asarray(perm)
    assert sorted(perm.tolist()) == list(range(nv))
    old = wb.poses[i, :nv].copy()
    wb.poses[i, perm] = old
    wb.r_idx[i, :nr, 0] = perm[wb.r_idx[i, :nr, 0]]
    pose1 = wb.r_idx[i, :nr, 1] >= 0
    wb.r_idx[i, :nr, 1][pose1] = perm[wb.r_idx[i, :nr, 1][pose1]]
    wb.p_idx[i, :npr] = perm[wb.p_idx[i, :npr]]
    wb.s_idx[i, :ns, :2] = perm[wb.s_idx[i, :ns, :2]]
    return wb


def shared_edges(wb, i):
    """result[6]: the binary edges whose (unordered) pair of poses carries another binary edge"""
    pairs = [(min(p), max(p)) for p in window_pairs(wb, i)]
    return sum(1 for p in pairs if pairs.count(p) > 1)


# ---- the natural-order fallback: a graph whose minimum-degree fill does not fit its handle --------------------------------------------------
def random_banded(rng):
    """one draw of the fallback search: (nv, pairs) of a random graph of 8 .. 64 poses inside a band of 2 .. 8"""
    nv, band, p = int(rng.integers(8, 65)), int(rng.integers(2, 9)), rng.uniform(0.2, 0.9)
    pairs = [(k - s, k) for k in range(nv) for s in range(1, band + 1) if k - s >= 0 and rng.random() < p]
    return nv, sorted(set(pairs + [(k - band, k) for k in range(band, nv, int(rng.integers(1, 6)))]))


@functools.lru_cache(maxsize=None)
def fallback_graph(draws=10000):
    """(draw, nv, band, pairs) of the first of `draws` random banded graphs whose minimum-degree fill exceeds the capacity a handle of exactly its
    size and band has (the kernel then falls back to the caller's order), or None"""
    from _elimination_model import nnz_capacity_blocks, order_small
    rng = np.random.default_rng(77)
    for d in range(draws):
        nv, pairs = random_banded(rng)
        band = max(abs(u - v) for u, v in pairs)
        if order_small(nv, pairs).nb > nnz_capacity_blocks((nv, 0, 0, 0, band)):
            return d, nv, band, pairs
    return None


# ---- the batches of tests/test_gpu_window_structures.py -------------------------------------------------------------------------------
# name -> (six_dof, bw_max, seed, windows); a window: (label, pairs, doubled pair numbers), or (label, ("arrow6", T, A)) for
# _general_cov_inputs.fill_arrowhead6.  Ragged on purpose: neighbouring workgroups take different structure branches.  The sizes are the ones
# at which tests/test_elimination_model_cpu.py finds every window on the branch it is listed for; the seeds the ones at which
# tests/test_graph_families_cpu.py found the reference stable under relabelling — fixed before the first GPU run.
SKY_SPANS = ((17, 5, 0), (40, 11, 3))
_FALLBACK = fallback_graph()
_TREE40 = random_tree(np.random.default_rng(1), 40)
BATCHES = {
    # arrays in LDS (14 slots: 224 stage-A records): clique 10 needs 221 of them, clique 12 needs 365
    "lds6": (True, -1, 7101, [("ring12", ring(12), (2,)), ("clique6", clique(6), ()), ("components14", components(14), ()), ("pad5", chain(5), ())]),
    "lds3": (False, -1, 7102, [("clique12", clique(12), ()), ("clique10", clique(10), ()), ("ring12", ring(12), ()), ("components14", components(14), (0, 9))]),
    # arrays in the workspace, one-word masks
    "ws6": (True, -1, 7103, [("ring20", ring(20), ()), ("grid6x6", grid(6, 6), (5,)), ("grid8x8", grid(8, 8), ()), ("tree40", _TREE40, ()),
                             ("chain30clique8", chain_with_clique(30, 8), ()), ("components24", components(24), ()), ("pad5", chain(5), ())]),
    "ws3": (False, -1, 7104, [("grid8x8", grid(8, 8), ()), ("ring20", ring(20), (3,)), ("chain30clique8", chain_with_clique(30, 8), ()),
                              ("components24", components(24), ())]),
    # eight-word masks, eight waves
    "wide6": (True, -1, 7105, [("ladder60", ladder(60), ()), ("grid8x16", grid(8, 16), ()), ("ring200", ring(200), (7,)), ("grid10x30", grid(10, 30), ()),
                               ("arrowhead70+6", arrowhead(70, 6), ()), ("arrowhead64+12", arrowhead(64, 12), ()), ("pendant", arrowhead_with_pendant(70, 6), ()), ("components130", components(130), ())]),
    "wide3": (False, -1, 7106, [("ladder60", ladder(60), ()), ("grid8x16", grid(8, 16), ()), ("ring200", ring(200), ()), ("grid10x30", grid(10, 30), (11,)),
                                ("pendant", arrowhead_with_pendant(70, 6), ()), ("components130", components(130), ())]),
    # anchor self-calibration windows (unknown anchors under weak position priors): analytic only — in numeric mode the reference alone moves by
    # 6e-7 .. 1e-5 m under relabelling on these (twelve seeds per shape: 22 of 24 above the 1e-6 m limit), which leaves no room under the 1e-5 m bound
    "selfcal6": (True, -1, 7111, [("arrow70+6", ("arrow6", 70, 6)), ("arrow64+12", ("arrow6", 64, 12))]),
    # a 66-slot handle: its dense list holds 132 entries
    "dense6": (True, -1, 7107, [("chain66clique48", chain_with_clique(66, 48), ()), ("chain60clique30", chain_with_clique(60, 30), ())]),
    "dense3": (False, -1, 7108, [("chain66clique48", chain_with_clique(66, 48), ()), ("chain60clique30", chain_with_clique(60, 30), ())]),
    # the skyline path
    "sky6": (True, 40, 7109, [("banded520", banded_with_long_links(520, SKY_SPANS), ())]),
}
if _FALLBACK is not None:
    # the search's graph in a handle of exactly its size and band, next to two windows whose minimum-degree order fits
    BATCHES["fallback6"] = (True, _FALLBACK[2], 7110, [("banded", _FALLBACK[3], ()), ("chain30", chain(30), ()), ("ladder10", ladder(10), (4,))])
NATURAL =("ws6", "ws3", "wide6", "wide3")          # the batches solved again in the caller's order
MODES = ("analytic", "numeric")


def batch_modes(name):
    return ("analytic",) if name == "selfcal6" else MODES

# (pose and rotation entries, chi2 relative): tests/test_gpu_window_parity.py's
TOL = {"analytic": (1e-7, 1e-6), "numeric": (1e-5, 1e-4)}


def window_spec(name, i):
    """(nv, pairs) of window i of batch `name` as the structure analysis sees it"""
    w = BATCHES[name][3][i]
    if isinstance(w[1], tuple) and w[1][0] == "arrow6":
        T, A = w[1][1:]
        return T + A, arrowhead(T, A)
    return pair_count(w[1]), w[1]


def batch_caps(name):
    """(nv_max, nr_max, np_max, ns_max, bw_max) of batch `name`: exactly what its largest window needs"""
    wb = build_batch(name)
    bw = BATCHES[name][1]
    return wb.caps + (wb.caps[0] - 1 if bw < 0 else bw,)


@functools.lru_cache(maxsize=None)
def _built(name):
    from localization_amd.window import WindowBatch
    six_dof, _, seed, windows = BATCHES[name]
    wb = None
    for caps in ((1024, 8192, 1024, 2048), None):   # first into roomy tables, then into tables of exactly the counts found
        if caps is None:
            caps = tuple(int(x) for x in wb.counts.max(axis=0))
        wb = WindowBatch(len(windows), *caps)
        for i, w in enumerate(windows):
            rng = np.random.default_rng(seed + 17 * i)
            if isinstance(w[1], tuple):
                fill_arrowhead6(wb, i, rng, *w[1][1:])
            else:
                fill_graph(wb, i, rng, pair_count(w[1]), w[1], six_dof, w[2])
    return wb


def build_batch(name):
    """a fresh copy of batch `name` (the same bits every time)"""
    import localization_amd as la
    return _built(name).copy()


def batch_perms(name):
    """per window the relabelling of the transparency checks: random; the skyline window is reversed (its band stays its band)"""
    wb = _built(name)
    rng = np.random.default_rng(BATCHES[name][2] + 1)
    if BATCHES[name][1] >= 0:
        return [np.arange(int(nv))[::-1].copy() for nv in wb.counts[:, 0]]
    return [rng.permutation(int(nv)) for nv in wb.counts[:, 0]]


def relabelled_batch(name):
    wb = build_batch(name)
    for i, perm in enumerate(batch_perms(name)):
        relabel(wb, i, perm)
    return wb


@functools.lru_cache(maxsize=None)
def oracle_solution(name, mode, relabelled=False):
    """[(poses [nv][12], chi2, outer iterations, LM trials)] per window: the oracle's 10 iterations in Jacobian mode `mode`.  Solved once per
    process and shared: treat as read-only."""
    from oracle import oracle as O
    from _oracle_window import oracle_solve_instance
    wb = relabelled_batch(name) if relabelled else build_batch(name)
    out = []
    for i in range(wb.B):
        poses, chi2, st = oracle_solve_instance(wb, i, ANCH, 10, O.JAC_ANALYTIC if mode == "analytic" else O.JAC_NUMERIC_G2O)
        poses.setflags(write=False)
        out.append((poses, chi2, int(st.outer_iterations), int(st.lm_trials)))
    return out
