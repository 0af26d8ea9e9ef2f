"""Test helper of tests/test_gpu_forest_groups_covariance.py: the mixed forest batches whose covariances option "forest_groups_covariance"
serves.  Built from tests/_forest_groups_cases.py; the solve tests' five_topologies() is not usable here — its rich 24-pose star leaves pose
12 alone with one range (H singular by the reference), and random_forest(33, 3) has one-pose trees.

Regularity of these inputs was checked on the CPU with the oracle and _covariance_ref.hessian (72 windows, of[b] = b % 6, mixed_batch seed
41, vary on and off, both Jacobian modes): the smallest relative LDL^T pivot of the reference's H is 4.0e-5 (topology 4), kappa <= 6.3e5 —
four orders clear of the 1e-9 line the forest tests hold their inputs to (test_inputs_are_regular_by_the_reference repeats it at the GPU's
poses)."""
import numpy as np

import _forest_groups_cases as FC
from _forest_groups_cases import ANCH, CAPS  # noqa: F401  (re-exported)

B, G = 72, 6
OF = [b % G for b in range(B)]          # neighbouring waves differ in topology
SEED = 41


def six_topologies():
    """1. star(64, 8); 2. the rich 24-pose star with pose 12 hung on its key (11) and the link between the keys 11 and 15 cut: two trees,
    0 ... 14 and 15 ... 23, smoothness ranges only where the parent is the previous pose; 3. star(40, 6) at another phase of the cadence;
    4. a key with three leaves, the smallest forest that is no chain; 5. a random forest of 33 poses with at least two anchor ranges per pose
    and the roots four (trees of 29 and 4 poses); 6. the two-pose window, the smallest forest"""
    rich = FC.star(24, 4, rich=True)
    rich["parent"][12] = 11
    rich["parent"][15] = -1
    rich["smooth"] = rich["smooth"] & (rich["parent"] == np.arange(24) - 1)
    rnd = FC.random_forest(33, 7)
    rnd["n_anchor"] = np.maximum(rnd["n_anchor"], 2)
    rnd["n_anchor"][rnd["parent"] < 0] = 4
    return [FC.star(64, 8), rich, FC.star(40, 6, first=2), FC.star(4, 4, n_anchor=2, lever=True), rnd,
            FC.star(2, 1, n_anchor=3, lever=True, reverse=True, prior_on=(1,))]


def mixed(la, vary, seed=SEED, of=OF, topos=None):
    return FC.mixed_batch(la, six_topologies() if topos is None else topos, of, seed, vary=vary)


def min_relative_pivot(H):
    """smallest LDL^T pivot of H_kept relative to its diagonal entry (natural order)"""
    keep = np.diag(H) != 0
    A = H[np.ix_(keep, keep)].copy()
    d0 = np.diag(A).copy()
    worst = np.inf
    for j in range(len(A)):
        worst = min(worst, A[j, j] / d0[j])
        if not A[j, j] > 0:
            return worst
        A[j + 1:, j + 1:] -= np.outer(A[j + 1:, j], A[j, j + 1:]) / A[j, j]
    return worst
