"""Test helper: the inputs of the structured-prior tests (option "prior_information_structured": wave3_lm_kernel<JAC, true> and
covariance_kernel<3, .., true>) — tests/test_structured_prior_cpu.py on the oracle and numpy alone, tests/test_gpu_structured_prior.py on the
GPU.  Translation-only chains of tests/_fixed_lag.py (Chain, add_chain_poses), eight windows per case, every prior with a row in the table
of full information matrices: a random symmetric positive semi-definite 3 x 3 block of rank 1, 2 or 3 on the translation, zeros elsewhere.

Magnitudes: the marginal prior of a dropped pose reaches its neighbour through one smoothness edge, so tests/_dense_prior_ref.marginal_ref's
eigenvalues on these chains lie below _fixed_lag.SMOOTH_INFO = 11.1; a block here is scale * A A^T with unit columns in A and
scale = SMOOTH_INFO * 10^u, u uniform in [-1.5, 1]: 0.35 .. 111.

p_val's diagonal is NaN in every case: with the table set nothing reads it — not the kernels, and not the structure test either (a test that
read it would call no batch here translation-only)."""
import numpy as np

import _fixed_lag as F

ANCH = F.ANCH


def caps(T, np_max, nr_max=None):
    return T, T * F.NA_MAX + 2 * max(T - 1, 0) if nr_max is None else nr_max, np_max, 0


def dense_info(rng, rank):
    A = rng.normal(size=(3, rank))
    A /= np.linalg.norm(A, axis=0)
    W3 = F.SMOOTH_INFO * 10.0 ** rng.uniform(-1.5, 1.0) * (A @ A.T)
    info = np.zeros((6, 6))
    info[:3, :3] = 0.5 * (W3 + W3.T)
    return info


def _spec(T, na, priors, **kw):
    return dict(T=T, na=na, priors=priors, **kw)


RANKS = (1, 2, 1, 3, 1, 2, 3, 1)   # of window i's (first) prior: the rank-1 ones — what a marginal usually is — in every other window

CASES = {
    # a lone pose; the first coupling
    "T1": [_spec(1, 3 + i % 2, [(0, RANKS[i])]) for i in range(8)],
    "T2": [_spec(2, 3 + i % 2, [(i % 2, RANKS[i])]) for i in range(8)],
    # the fixed-lag shape: W = 16, four speculative groups, dual scoring (<= 29 edges, one prior)
    "T6": [_spec(6, 3 + i % 2, [(0, RANKS[i])]) for i in range(8)],
    # 49 edges: no dual scoring, four groups
    "T10": [_spec(10, 4, [(0, RANKS[i])]) for i in range(8)],
    # W = 32: two groups
    "T20": [_spec(20, 3 + i % 2, [(0, RANKS[i])]) for i in range(8)],
    # W = 64, no speculation; 80 priors: the q += 64 prior loop and the > 64 edges split
    "T40x2": [_spec(40, 3 + i % 2, [(k, 1 + (k + i + j) % 3) for k in range(40) for j in range(2)]) for i in range(8)],
    # (three anchors per pose and edge tables of exactly 3 * 64 + 63 rows: wave3_lm_kernel keeps a window's edge records in 64 KiB of LDS)
    "T64": [_spec(64, 3, [(0, RANKS[i]), (63, RANKS[7 - i])]) for i in range(8)],
    # a second smoothness edge on one pair, stored the other way round: rank1 == false
    "doubled": [_spec(10, 3 + i % 2, [(0, RANKS[i])], doubled=(3,)) for i in range(8)],
    "missing": [_spec(10, 3 + i % 2, [(0, RANKS[i])], missing=(4,)) for i in range(8)],
    "ragged": [_spec((1, 6, 10, 6, 1, 10, 6, 10)[i], 3 + i % 2, [(0, RANKS[i])]) for i in range(8)],
    # a diagonal-style prior (a lidar z prior expressed in the table) and a dense one on the same pose, in either order
    "zprior": [_spec(10, 3 + i % 2, [(0, "z"), (0, RANKS[i])] if i % 2 == 0 else [(0, RANKS[i]), (0, "z")]) for i in range(8)],
    # windows whose table row is all zeros (the marginal pass's "plain drop")
    "zero": [_spec(6, 3 + i % 2, [(0, "zero" if i % 2 == 0 else RANKS[i])]) for i in range(8)],
    # covariances: window 3 is singular — EVERY pose keeps one anchor range (tests/_fixed_lag.py's "one_range", extended to every pose:
    # 2 T - 1 rank-one terms and a rank-1 prior for 3 T translations)
    "singular": [_spec(6, 3 + i % 2, [(0, 1 if i == 3 else RANKS[i])], singular=i == 3) for i in range(8)],
}
NR_MAX = {"T64": 3 * 64 + 63}
SEED = {name: 8300 + 10 * k for k, name in enumerate(CASES)}
# Window i's trajectory is Chain(SEED[name] + i), but for five windows that take the next seed in steps of 1000: on the first, the ORACLE's
# own ten-iteration solves in its two Jacobian modes end more than NUMERIC_GAP apart (1.0e-6 .. 3.1e-6 m).  Such a window amplifies the
# 1e-7 relative noise of g2o's difference quotient — through an LM accept / reject decision that sits on the edge — to within a factor ten
# of the numeric mode's 1e-5 m tolerance, whoever evaluates the quotient; tests/test_structured_prior_cpu.py holds every window to the bound
# on the oracle alone.
NUMERIC_GAP = 1e-6
CHAIN_SEED = {name: [SEED[name] + i for i in range(8)] for name in CASES}
for _name, _i in (("T1", 4), ("T40x2", 6), ("T64", 4), ("ragged", 2), ("zero", 6)):
    CHAIN_SEED[_name][_i] += 1000
SINGULAR = {"singular": (3,)}   # the windows built to be singular: excluded from every comparison, by name
COV_CASES = ("T2", "T6", "T10", "T64", "T40x2")


def case_batch(la, name):
    specs = CASES[name]
    T = max(s["T"] for s in specs)
    wb = la.WindowBatch(len(specs), *caps(T, max(len(s["priors"]) for s in specs), NR_MAX.get(name)))
    rng = np.random.default_rng(SEED[name] + 5)
    for i, s in enumerate(specs):
        ch = F.Chain(CHAIN_SEED[name][i], s["T"], s["na"])
        F.add_chain_poses(wb, i, ch, 0, s["T"], doubled=s.get("doubled", ()), missing=s.get("missing", ()),
                          keep_ranges={k: 1 for k in range(s["T"])} if s.get("singular") else None)
        for slot, kind in s["priors"]:
            if kind == "z":
                wb.add_prior(i, slot, np.array([ch.est[slot, 0], ch.est[slot, 1], ch.truth[slot, 2] + rng.normal(0, 0.02)]), np.eye(3), np.array([0, 0, 1 / 0.05, 0, 0, 0.0]))
            else:
                info = np.zeros((6, 6)) if kind == "zero" else dense_info(rng, kind)
                wb.add_prior(i, slot, ch.truth[slot] + rng.normal(0, 0.05, 3), np.eye(3), info=info)
    if wb.p_info is None:
        wb.p_info = np.zeros((wb.B, max(wb.caps[2], 1), 36))
    wb.p_val[:, :, 12:] = np.nan
    return wb


def diagonal_batch(la):
    """ten-pose chains with DIAGONAL priors alone and no table: a lidar z prior on pose 0, a position prior on pose 3"""
    wb = la.WindowBatch(8, *caps(10, 2))
    rng = np.random.default_rng(8295)
    for i in range(8):
        ch = F.Chain(8280 + i, 10, 3 + i % 2)
        F.add_chain_poses(wb, i, ch, 0, 10)
        wb.add_prior(i, 0, np.array([ch.est[0, 0], ch.est[0, 1], ch.truth[0, 2] + rng.normal(0, 0.02)]), np.eye(3), np.array([0, 0, 1 / 0.05, 0, 0, 0.0]))
        wb.add_prior(i, 3, ch.truth[3] + rng.normal(0, 0.05, 3), np.eye(3), np.array([30.0, 7.0, 12.0, 0, 0, 0]))
    return wb
