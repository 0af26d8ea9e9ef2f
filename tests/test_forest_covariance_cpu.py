"""The selected inversion forest_covariance_kernel.hip runs, stated in numpy on a random forest H and compared with the dense inverse:
with every node eliminated before its parent the factor has no fill, so upwards S_c = H_cc - sum_k K_k H_kc, K_c = H_pc S_c^-1 and
downwards Sigma_r = S_r^-1, Sigma_c = S_c^-1 + K_c^T Sigma_p K_c give the diagonal blocks of H^-1."""
import numpy as np
import pytest


def _forest_blocks(H, parent, order, D=6):
    nv = len(parent)
    blk = lambda a, b: H[D * a:D * a + D, D * b:D * b + D]
    S = [blk(v, v).copy() for v in range(nv)]
    K = [None] * nv
    for v in order:                      # children before their parent
        S[v] = np.linalg.inv(S[v])
        p = parent[v]
        if p >= 0:
            K[v] = blk(p, v) @ S[v]
            S[p] -= K[v] @ blk(v, p)
    for v in order[::-1]:                # parents before their children
        p = parent[v]
        if p >= 0:
            S[v] = S[v] + K[v].T @ S[p] @ K[v]
    return S


@pytest.mark.parametrize("seed,nv", [(0, 2), (1, 7), (2, 24), (3, 64)])
def test_two_sweeps_give_the_diagonal_blocks_of_the_inverse(seed, nv):
    rng = np.random.default_rng(seed)
    D = 6
    parent = np.full(nv, -1)
    roots = {0} | ({int(rng.integers(1, nv))} if nv > 4 else set())
    for v in range(1, nv):
        if v not in roots:
            parent[v] = int(rng.integers(0, v))
    H = np.zeros((D * nv, D * nv))
    for v in range(nv):                  # a unary factor per pose, a binary factor per (child, parent) pair
        A = rng.normal(size=(D, D))
        H[D * v:D * v + D, D * v:D * v + D] += A @ A.T + 0.5 * np.eye(D)
        p = parent[v]
        if p >= 0:
            J = rng.normal(size=(D, 2 * D))
            ix = np.r_[D * v:D * v + D, D * p:D * p + D]
            H[np.ix_(ix, ix)] += J.T @ J
    # any order with children before their parent: here by decreasing depth
    depth = np.zeros(nv, dtype=int)
    for v in range(nv):
        if parent[v] >= 0:
            depth[v] = depth[parent[v]] + 1
    order = sorted(range(nv), key=lambda v: -depth[v])
    got = _forest_blocks(H, parent, order)
    want = np.linalg.inv(H)
    for v in range(nv):
        w = want[D * v:D * v + D, D * v:D * v + D]
        assert np.linalg.norm(got[v] - w) <= 1e-10 * np.linalg.norm(w)
