"""Test helper of the joint covariance tests (tests/test_joint_covariance_cpu.py, tests/test_gpu_joint_covariance.py): the reference blocks
[H^-1]_ij, the error of a block, and numpy models of how the four covariance passes form a cross block ("Joint marginals").

Every model takes H [6 nv][6 nv] (tests/_covariance_ref.hessian) with the diagonal of every excluded coordinate set to 1, as the kernels
do, and returns the 6 x 6 block (i, j) of its inverse; the rows / columns of excluded coordinates are dropped by the caller."""
import numpy as np


def blk(M, i, j, d=6):
    return M[d * i:d * i + d, d * j:d * j + d]


def kept_inverse(H):
    """(H^-1 on the kept coordinates, 0 elsewhere; keep): the reference of every block"""
    keep = np.diag(H) != 0.0
    Sig = np.zeros_like(H)
    Sig[np.ix_(keep, keep)] = np.linalg.inv(H[np.ix_(keep, keep)])
    return Sig, keep


def unit_excluded(H):
    keep = np.diag(H) != 0.0
    Hm = H.copy()
    Hm[~keep, ~keep] = 1.0
    return Hm


def block_error(G, Sig, i, j):
    """||G_ij - R_ij||_F / sqrt(||R_ii||_F ||R_jj||_F): a cross block can be arbitrarily small, so its own norm is no scale"""
    return np.linalg.norm(G - blk(Sig, i, j)) / np.sqrt(np.linalg.norm(blk(Sig, i, i)) * np.linalg.norm(blk(Sig, j, j)))


def pose_pairs(wb, i):
    nr, ns = int(wb.counts[i, 1]), int(wb.counts[i, 3])
    out = [(int(wb.r_idx[i, e, 0]), int(wb.r_idx[i, e, 1])) for e in range(nr) if wb.r_idx[i, e, 1] >= 0]
    return out + [(int(wb.s_idx[i, e, 0]), int(wb.s_idx[i, e, 1])) for e in range(ns)]


def forest_parents(nv, edges):
    """parent slot per pose (-1: a root) of the forest the pose-to-pose edges form, every tree rooted at its smallest slot"""
    adj = [set() for _ in range(nv)]
    for u, v in edges:
        adj[u].add(v); adj[v].add(u)
    parent, seen = [-1] * nv, [False] * nv
    for root in range(nv):
        if seen[root]:
            continue
        seen[root] = True
        todo = [root]
        while todo:
            u = todo.pop()
            for v in sorted(adj[u]):
                if not seen[v]:
                    seen[v] = True; parent[v] = u; todo.append(v)
    return parent


class ForestModel:
    """The forest pass: S_c = H_cc - sum_children K_k H_kc, K_c = H_pc S_c^-1 upwards; Sigma_c = S_c^-1 + K_c^T Sigma_p K_c downwards;
    Sigma_ij = M_i Sigma_aa M_j^T through the lowest common ancestor a, M = the product of -K^T along the path.  A chain is the forest with
    parent = next pose."""

    def __init__(self, H, parent, d=6):
        nv = len(parent)
        self.parent, self.d = parent, d
        depth = [0] * nv
        for v in range(nv):
            u = v
            while parent[u] >= 0:
                u = parent[u]; depth[v] += 1
        self.depth = depth
        order = sorted(range(nv), key=lambda v: -depth[v])   # children before their parent
        S = [blk(H, v, v, d).copy() for v in range(nv)]
        self.K = [None] * nv
        for v in order:
            S[v] = np.linalg.inv(S[v])
            p = parent[v]
            if p >= 0:
                Hpv = blk(H, p, v, d)
                self.K[v] = Hpv @ S[v]
                S[p] = S[p] - self.K[v] @ Hpv.T
        self.Sigma = S
        for v in reversed(order):
            p = parent[v]
            if p >= 0:
                self.Sigma[v] = S[v] + self.K[v].T @ self.Sigma[p] @ self.K[v]

    def _path(self, v, a):
        M = np.eye(self.d)
        steps = []
        while v != a:
            steps.append(v); v = self.parent[v]
        for u in steps:             # M = (-K_v^T)(-K_{p(v)}^T) ...
            M = M @ (-self.K[u].T)
        return M

    def cross(self, i, j):
        a, b = i, j
        while a != b and a >= 0 and b >= 0:
            if self.depth[a] >= self.depth[b]: a = self.parent[a]
            else: b = self.parent[b]
        if a < 0 or a != b:
            return np.zeros((self.d, self.d))
        return self._path(i, a) @ self.Sigma[a] @ self._path(j, a).T


def chain_cross(H, nv, i, j, d=6):
    """The chain pass: Sigma_ij = (-K_i^T) .. (-K_{j-1}^T) Sigma_jj for i < j, on the block-tridiagonal recurrences"""
    m = ForestModel(H, [v + 1 if v + 1 < nv else -1 for v in range(nv)], d)
    if i > j:
        return chain_cross(H, nv, j, i, d).T
    R = m.Sigma[j]
    for k in range(j - 1, i - 1, -1):
        R = -m.K[k].T @ R
    return R


def arrow_cross(H, nv, nb, i, j):
    """The arrowhead pass on the translation coordinates (3 x 3 blocks): border = the last nb slots, Y = A^-1 B, S = C - B^T Y;
    border - border: S^-1; chain i - border: -Y_i S^-1; chain - chain: [A^-1]_ij + Y_i S^-1 Y_j^T with [A^-1]_ij by the chain recipe on A.
    Returns the 6 x 6 block (rotation rows / columns 0)."""
    t = np.array([6 * v + k for v in range(nv) for k in range(3)])
    H3 = H[np.ix_(t, t)]
    nc = nv - nb
    A, B, C = H3[:3 * nc, :3 * nc], H3[:3 * nc, 3 * nc:], H3[3 * nc:, 3 * nc:]
    Y = np.linalg.solve(A, B)
    Sinv = np.linalg.inv(C - B.T @ Y)
    Yb = lambda v: Y[3 * v:3 * v + 3]
    lo, hi = min(i, j), max(i, j)
    if lo >= nc:
        X = blk(Sinv, lo - nc, hi - nc, 3)
    elif hi >= nc:
        X = -Yb(lo) @ Sinv[:, 3 * (hi - nc):3 * (hi - nc) + 3]
    else:
        X = chain_cross(A, nc, lo, hi, 3) + Yb(lo) @ Sinv @ Yb(hi).T
    out = np.zeros((6, 6))
    out[:3, :3] = X if i <= j else X.T
    return out


def envelope_inverse(H, first):
    """The envelope pass: block LDL^T and selected inversion restricted to the envelope first[] (tests/_general_cov_inputs.py:
    envelope_selected_inverse, which returns the diagonal blocks alone); every block outside the envelope stays NaN.  Returns the work
    array: block (i, j), first[i] <= j <= i, holds [H^-1]_ij."""
    nv = len(first)
    W = np.full_like(H, np.nan)
    for i in range(nv):
        for j in range(first[i], i + 1):
            blk(W, i, j)[:] = blk(H, i, j)
    struct = [[k for k in range(j + 1, nv) if first[k] <= j] for j in range(nv)]
    for j in range(nv):
        Sinv = np.linalg.inv(blk(W, j, j))
        col = {k: blk(W, k, j).copy() for k in struct[j]}
        for k in struct[j]:
            blk(W, k, j)[:] = col[k] @ Sinv
        for a, ka in enumerate(struct[j]):
            for kb in struct[j][:a + 1]:
                blk(W, ka, kb)[:] -= blk(W, ka, j) @ col[kb].T
        blk(W, j, j)[:] = Sinv
    for j in range(nv - 1, -1, -1):
        sig = lambda i, k: blk(W, i, k) if i >= k else blk(W, k, i).T
        new = {i: -sum(sig(i, k) @ blk(W, k, j) for k in struct[j]) for i in struct[j]}
        blk(W, j, j)[:] -= sum((blk(W, k, j).T @ new[k] for k in struct[j]), np.zeros((6, 6)))
        for i in struct[j]:
            blk(W, i, j)[:] = new[i]
    return W


def envelope_cross(W, i, j):
    return blk(W, i, j).copy() if i >= j else blk(W, j, i).T.copy()


def envelope_blocks_with_pairs(wb, i, pairs):
    """the envelope of window i in blocks with the requested pairs taken as edges (the Python profile model of loc_window_joint_covariance_plan)"""
    import _general_cov_inputs as G
    nv = int(wb.counts[i, 0])
    first = G.envelope_first(nv, G.window_pairs(wb, i) + [(int(a), int(b)) for a, b in pairs])
    return int((np.arange(nv) - first + 1).sum())
