"""Test helper: the inputs of the edge-audit tests (tests/test_edge_audit_cpu.py on the oracle alone, tests/test_gpu_edge_audit.py on the GPU),
built from the project's existing builders: tests/_fixed_lag.py (translation-only chains), tests/_general_cov_inputs.py (6-DoF and long
chains), tests/_arrow_cov_inputs.py (arrowheads) and the twist / forest helpers of the GPU covariance tests (imported only by the audit cases
that need them: those modules are GPU test files).

The prune inputs are chains of ten poses with four anchors per pose (sigma 0.03 m) and nine smoothness edges: 49 range rows.  PRUNE_MIN_EDGES
is 49, so a plain window sits AT the threshold (active == min_edges: the rule keeps everything, whatever its outliers) and a window with one
doubled smoothness edge one above it.  Planted outliers: anchor ranges displaced by +1.5 m (50 sigma)."""
import numpy as np

import _fixed_lag as F
import _general_cov_inputs as G
import _arrow_cov_inputs as A

PRUNE_CHI2_MAX = 2.0      # the reference's constant (localization.cpp:172-181)
PRUNE_MIN_EDGES = 49      # (the reference's is 100: the windows here are sized to sit on both sides of 49)
PRUNE_T = 10
DISPLACED = 1.5


def prune_batch(la, seed=9700, B=8):
    """(batch, planted [B][nr_max] bool): window 0: 49 active rows (== min_edges), outliers planted; window 1: 50 (== min_edges + 1), outliers
    planted; window 2: 50 rows of which one anchor range has information 0.0 — the caller's own level 1 — and a residual of 1.5 m: 49 active,
    kept whole; window 3: 50 rows, no outlier; windows 4 ..: 50 rows, two or three outliers, one of them on the newest pose"""
    wb = la.WindowBatch(B, *F.window_caps(PRUNE_T))
    planted = np.zeros((B, wb.caps[1]), dtype=bool)
    for i in range(B):
        ch = F.Chain(seed + i, PRUNE_T, 4)
        F.add_chain_poses(wb, i, ch, 0, PRUNE_T, doubled=() if i == 0 else (1,))
        nr = int(wb.counts[i, 1])
        anchor_rows = [e for e in range(nr) if wb.r_idx[i, e, 1] < 0]
        picks = [] if i == 3 else [anchor_rows[(5 + 7 * i) % len(anchor_rows)], anchor_rows[-1 - (i % 3)]] + ([anchor_rows[11]] if i % 2 else [])
        if i == 2:
            picks = picks[:1]
        for e in picks:
            wb.r_val[i, e, 0] += DISPLACED
            planted[i, e] = True
        if i == 2:
            wb.r_val[i, picks[0], 1] = 0.0
            planted[i, picks[0]] = False
    return wb, planted


def _symmetric_table(wb, rng):
    """a full 6 x 6 information matrix for every prior of the batch (exactly symmetric, positive definite, of the diagonal's size)"""
    wb.p_info = np.zeros((wb.B, max(wb.caps[2], 1), 36))
    for i in range(wb.B):
        for e in range(int(wb.counts[i, 2])):
            M = rng.normal(size=(6, 6)); W = M @ M.T + 6 * np.eye(6)
            W = (W + W.T) * 0.5
            wb.p_info[i, e] = (W * (max(wb.p_val[i, e, 12:].max(), 1.0) / np.trace(W))).reshape(36)
    return wb


def _endpoint1_arms(wb):
    """endpoint-1 lever arms on every other anchor range (the anchor's own antenna) and on every pose-to-pose range (a peer's antenna)"""
    wb.r_off1 = np.zeros((wb.B, max(wb.caps[1], 1), 3))
    for i in range(wb.B):
        for e in range(int(wb.counts[i, 1])):
            if wb.r_idx[i, e, 1] >= 0: wb.r_off1[i, e] = (-0.08, 0.03, 0.02)
            elif e % 2: wb.r_off1[i, e] = (0.05, -0.02, 0.1)
    return wb


def _ragged(la):
    """four windows on one handle: a chain of ten, a window of ONE pose (nv = 1), a window WITHOUT range rows (nr = 0: three poses, a z prior
    each on two of them) and a chain of four"""
    wb = la.WindowBatch(4, *F.window_caps(10))
    F.add_chain_poses(wb, 0, F.Chain(9801, 10, 4), 0, 10)
    F.add_chain_poses(wb, 1, F.Chain(9802, 1, 5), 0, 1)
    ch = F.Chain(9803, 3, 3)
    for s in range(3): wb.add_pose(2, ch.est[s])
    for s in (0, 2): wb.add_prior(2, s, np.array([ch.est[s, 0], ch.est[s, 1], ch.truth[s, 2]]), np.eye(3), np.array([0, 0, 1 / 0.05, 0, 0, 0.0]))
    F.add_chain_poses(wb, 3, F.Chain(9804, 4, 3), 0, 4, doubled=(1,))
    assert wb.counts[2, 1] == 0 and wb.counts[1, 0] == 1
    return wb


def audit_case(la, name):
    """(batch, anchors, handle options {name: value}, the solve kernel a default resident solve of it takes or None)"""
    if name == "chain3_10":
        return F.first_window(la, [F.Chain(9600 + i, 10, 3 + i % 3) for i in range(8)], 10), F.ANCH, {}, "wave3_lm_kernel"
    if name == "chain6_12":
        return G.chain_batch(la, 9610, 6, 12, True), G.ANCH, {}, "wave6_lm_kernel"
    if name == "twist_15":
        from test_gpu_covariance import _twist_batch
        from test_gpu_window_parity import ANCH
        return _twist_batch(la, np.random.default_rng(9620), 6, 15, True), ANCH, {}, None
    if name == "forest_24":
        from test_gpu_forest_covariance import _two_trees
        from test_gpu_tree_parity import ANCH, _forest_batch
        return _two_trees(_forest_batch(la, np.random.default_rng(8101), 12, 24, 4, True)), ANCH, {"chain_min_batch": 1}, None
    if name == "endpoint1":
        return _endpoint1_arms(G.chain_batch(la, 9640, 5, 8, True, ragged=False)), G.ANCH, {}, "window_lm_kernel"
    if name == "table":
        return _symmetric_table(G.chain_batch(la, 9650, 5, 8, True, ragged=False), np.random.default_rng(9651)), G.ANCH, {}, "window_lm_kernel"
    if name == "chain_70":   # 70 * 4 + 69 = 349 range rows (5 full chunks of 64 and 29 more) and 35 priors in the even windows
        return G.chain_batch(la, 9660, 3, 70, False, ragged=False), G.ANCH, {}, None
    if name == "arrow_5_1":
        return A.case_batch(la, "5_1"), A.SURVEYED, {"arrow3": 1}, "arrow3_lm_kernel"
    if name == "ragged":
        return _ragged(la), F.ANCH, {}, None
    raise KeyError(name)


AUDIT_CASES = ["chain3_10", "chain6_12", "twist_15", "forest_24", "endpoint1", "table", "chain_70", "arrow_5_1", "ragged"]


def permuted(la, wb, order):
    return wb.take(order)
