"""Test helper: arrowhead (anchor self-calibration) windows whose UNDAMPED H is regular, for the covariance tests of
arrow_covariance_kernel.hip (tests/test_gpu_arrow_covariance.py on the GPU, tests/test_arrow_covariance_cpu.py on the oracle alone).

The generator follows test_gpu_arrow3_parity._arrow_batch (slot order: tag poses first, unknown anchors last; the same rich variations)
with one difference that the covariance needs and the solve does not: _arrow_batch's rich mode drops instances to A - 2 unknown anchors,
and a tag pose that ranges two nodes only leaves H rank-deficient by count (3T + 5 terms for 3T + 6 unknowns).  Here every tag pose ranges
at least FOUR nodes, unknown and surveyed together — poses that see fewer unknown anchors range surveyed ones instead — and every unknown
anchor carries its prior.  The surveyed table is test_gpu_arrow3_parity.FIXED and two more anchors (four nodes must exist when A = 1)."""
import numpy as np

FIXED = np.array([[4.0, -4.0, 0.5], [-4.0, 4.0, 2.5]])   # test_gpu_arrow3_parity.FIXED (that module is a GPU test file: not imported by the CPU test)
SURVEYED = np.vstack([FIXED, [[4.0, 4.0, 3.0], [-4.0, -4.0, 0.2]]])
MIN_NODES = 4


def arrow_cov_batch(la, rng, B, T, A, rich):
    """B hypotheses of up to T tag poses and up to A unknown anchors.  rich: ragged trajectory lengths and border sizes inside the batch, a
    missing smoothness link, ranges stored border-first, doubled (pose, anchor) ranges, missed ranges, ranges between unknown anchors, ranges
    to surveyed anchors, z priors on some tag poses."""
    nr_max = T * (A + MIN_NODES + 3) + A * A + 4
    wb = la.WindowBatch(B, T + A, nr_max, A + T, 0)
    true_anchors = np.column_stack([rng.uniform(-4, 4, A), rng.uniform(-4, 4, A), rng.uniform(0, 3, A)])
    tt = np.cumsum(rng.normal(0, 0.05, (T, 3)), axis=0) + np.array([0.0, 0.0, 1.2])
    for i in range(B):
        Ti = max(T - (3 * i) % 7, 4) if rich else T
        Ai = max(A - i % 3, 1) if rich else A
        hyp = true_anchors[:Ai] + rng.normal(0, 1.0, (Ai, 3))
        et = tt[:Ti] + rng.normal(0, 0.05, (Ti, 3))
        for k in range(Ti): wb.add_pose(i, et[k])
        for a in range(Ai):
            wb.add_pose(i, hyp[a]); wb.add_prior(i, Ti + a, hyp[a], np.eye(3), np.array([1.0, 1.0, 1.0, 0, 0, 0]))
        for k in range(Ti):
            nodes = 0
            for a in range(Ai):
                if rich and (k + a + i) % 11 == 0:
                    continue                                                  # a missed range
                nodes += 1
                d = float(np.float32(np.linalg.norm(tt[k] - true_anchors[a]) + rng.normal(0, 0.03)))
                if rich and (k + a) % 13 == 5:
                    wb.add_range(i, Ti + a, k, d, 1 / 0.055 ** 2)             # stored the other way round
                else:
                    wb.add_range(i, k, Ti + a, d, 1 / 0.055 ** 2)
                if rich and (k * 7 + a) % 29 == 3:
                    wb.add_range(i, k, Ti + a, d + 0.01, 0.5 / 0.055 ** 2)    # a second range on the same (pose, anchor) pair
            surveyed = [(k + j) % len(SURVEYED) for j in range(max(MIN_NODES - nodes, 0))]
            if rich and k % 5 == 0 and not surveyed:
                surveyed = [k % 2]
            for f in surveyed:
                wb.add_range(i, k, f, float(np.float32(np.linalg.norm(tt[k] - SURVEYED[f]) + rng.normal(0, 0.03))), 1 / 0.055 ** 2, anchor=True)
            if k and not (rich and i % 4 == 1 and k == Ti // 2):
                wb.add_range(i, k - 1, k, 0.0, 1 / (5.0 / 32 / 3) ** 2)
            if rich and k % 9 == 4:
                wb.add_prior(i, k, np.array([et[k, 0], et[k, 1], tt[k, 2]]), np.eye(3), np.array([0, 0, 1 / 0.05, 0, 0, 0.0]))
        if rich:
            for a in range(1, Ai):                                            # ranges between unknown anchors; one pair twice
                b = (a * 5 + i) % a
                wb.add_range(i, Ti + a, Ti + b, float(np.linalg.norm(true_anchors[a] - true_anchors[b]) + rng.normal(0, 0.03)), 1 / 0.055 ** 2)
            if Ai > 1:
                wb.add_range(i, Ti, Ti + 1, float(np.linalg.norm(true_anchors[0] - true_anchors[1])), 1 / 0.1 ** 2)
            wb.add_range(i, Ti + Ai - 1, 0, float(np.linalg.norm(true_anchors[Ai - 1] - SURVEYED[0])), 1 / 0.055 ** 2, anchor=True)
    return wb


def cut_gauge(wb, i):
    """window i keeps its structure but loses the information of its priors and of its ranges to surveyed anchors"""
    wb.p_val[i, :, 12:] = 0.0
    nr = int(wb.counts[i, 1])
    wb.r_val[i, :nr, 1] = np.where(wb.r_idx[i, :nr, 1] < 0, 0.0, wb.r_val[i, :nr, 1])


# The parity cases: (T, A, rich, option "arrow3" (None: a default handle), Jacobians, windows).  Seeds fixed after the regularity check of
# tests/test_arrow_covariance_cpu.py passed at the oracle-solved poses.
CASES = {
    "5_1": (5, 1, True, 1, ("analytic",), 7),
    "24_4": (24, 4, True, 1, ("analytic", "numeric"), 7),
    "70_6": (70, 6, True, 1, ("numeric",), 4),
    "40_12": (40, 12, True, 1, ("analytic",), 4),
    "130_4": (130, 4, True, None, ("numeric",), 3),
}


def case_batch(la, name):
    T, A, rich, _, _, B = CASES[name]
    return arrow_cov_batch(la, np.random.default_rng(9000 + 100 * T + A), B, T, A, rich)


def min_relative_pivot(H):
    """smallest LDL^T pivot of H_kept relative to its diagonal entry (natural order)"""
    keep = np.diag(H) != 0
    M = H[np.ix_(keep, keep)].copy()
    d0 = np.diag(M).copy()
    worst = np.inf
    for j in range(len(M)):
        worst = min(worst, M[j, j] / d0[j])
        if not M[j, j] > 0:
            return worst
        M[j + 1:, j + 1:] -= np.outer(M[j + 1:, j], M[j, j + 1:]) / M[j, j]
    return worst


def ranged_nodes(wb, i):
    """per tag pose of window i: how many distinct nodes (unknown anchors, surveyed anchors) it ranges; and the unknown anchors' slots"""
    nv, nr = int(wb.counts[i, 0]), int(wb.counts[i, 1])
    anchors = sorted({int(wb.p_idx[i, e]) for e in range(int(wb.counts[i, 2])) if wb.p_val[i, e, 12:15].all()})   # a prior on x, y and z
    seen = [set() for _ in range(nv)]
    for e in range(nr):
        v0, v1 = int(wb.r_idx[i, e, 0]), int(wb.r_idx[i, e, 1])
        if v1 < 0: seen[v0].add(v1)
        elif v1 in anchors and v0 not in anchors: seen[v0].add(v1)
        elif v0 in anchors and v1 not in anchors: seen[v1].add(v0)
    return [len(seen[v]) for v in range(nv) if v not in anchors], anchors
