"""Test helper: the per-edge chi2 audit and the removal rule of loc_window_edge_chi2_* / loc_window_prune_resident ("Edge audit
and outlier removal") by the CPU oracle and numpy alone.  The window is built in the oracle's general graph exactly as tests/_oracle_window.py
builds it (endpoint-1 lever arms included; a prior takes the row of the batch's p_info table when there is one), at given poses; every edge's
error comes from Graph.linearize(k) — edge order: ranges, then priors, then EdgeSE3 — and e^T Omega e is formed in numpy."""
import numpy as np


def _graph(wb, i, anchors, poses):
    from oracle import oracle as O
    nv, nr, np_, ns = (int(x) for x in wb.counts[i])
    G = O.Graph()
    anchors = np.asarray(anchors, dtype=float).reshape(-1, 3)
    for m, a in enumerate(anchors):
        G.add_vertex(m, a, fixed=True)
    base = 1000
    for k in range(nv):
        G.add_vertex(base + k, poses[k, 9:], poses[k, :9].reshape(3, 3))
    infos = []
    for e in range(nr):
        v0, v1 = int(wb.r_idx[i, e, 0]), int(wb.r_idx[i, e, 1])
        o1 = None if getattr(wb, "r_off1", None) is None else wb.r_off1[i, e].copy()
        G.add_range_edge(base + v0, (-1 - v1) if v1 < 0 else base + v1, wb.r_val[i, e, 0], wb.r_val[i, e, 1], off0=wb.r_val[i, e, 2:5].copy(), off1=o1)
        infos.append(np.array([[wb.r_val[i, e, 1]]]))
    for e in range(np_):
        Ri = wb.p_val[i, e, :9].reshape(3, 3); ti = wb.p_val[i, e, 9:12]
        W = np.diag(wb.p_val[i, e, 12:18]) if getattr(wb, "p_info", None) is None else wb.p_info[i, e].reshape(6, 6).copy()
        G.add_prior_edge(base + int(wb.p_idx[i, e]), -Ri.T @ ti, Ri.T, W)
        infos.append(W)
    for e in range(ns):
        Ri = wb.s_val[i, e, :9].reshape(3, 3); ti = wb.s_val[i, e, 9:12]
        W = wb.s_val[i, e, 12:].reshape(6, 6)
        G.add_se3_edge(base + int(wb.s_idx[i, e, 0]), base + int(wb.s_idx[i, e, 1]), -Ri.T @ ti, Ri.T, W, bool(wb.s_idx[i, e, 2]))
        infos.append(W)
    return G, infos


def window_chi2(wb, i, anchors, poses=None):
    """(r_chi2 [nr], p_chi2 [np], s_chi2 [ns], total, active, the oracle's own all-edges chi2 at the same poses) of window i at `poses`
    (default wb.poses[i])"""
    poses = wb.poses[i] if poses is None else poses
    nv, nr, np_, ns = (int(x) for x in wb.counts[i])
    G, infos = _graph(wb, i, anchors, poses)
    chi = np.zeros(len(infos))
    for k, W in enumerate(infos):
        err = G.linearize(k)[0]
        chi[k] = err @ W @ err
    active = int(np.count_nonzero(wb.r_val[i, :nr, 1] != 0.0)) + np_ + ns
    # (linearize has evaluated every edge at these poses, so og_chi2's sum over the edges' stored errors is the sum at them too)
    return chi[:nr], chi[nr:nr + np_], chi[nr + np_:], float(chi.sum()), active, (G.chi2() if len(infos) else 0.0)


def batch_chi2(wb, anchors, poses=None):
    """the outputs of loc_window_edge_chi2_host for the whole batch, padded with zeros: (r_chi2 [B][nr_max], p_chi2 [B][np_max], s_chi2
    [B][ns_max], total [B], active int32 [B])"""
    B = wb.B
    r = np.zeros((B, max(wb.caps[1], 1))); p = np.zeros((B, max(wb.caps[2], 1))); s = np.zeros((B, max(wb.caps[3], 1)))
    total = np.zeros(B); active = np.zeros(B, dtype=np.int32)
    for i in range(B):
        ri, pi, si, total[i], active[i], _ = window_chi2(wb, i, anchors, None if poses is None else poses[i])
        r[i, :len(ri)] = ri; p[i, :len(pi)] = pi; s[i, :len(si)] = si
    return r, p, s, total, active


def prune_flags(wb, r_chi2, active, chi2_max, min_edges):
    """(removed int32 [B][nr_max], n_removed int32 [B]) by the rule: a window with active > min_edges loses every range row with information
    != 0 and chi2 > chi2_max (both strict; NaN compares false)"""
    removed = np.zeros(r_chi2.shape, dtype=np.int32)
    for i in range(wb.B):
        nr = int(wb.counts[i, 1])
        if active[i] > min_edges:
            with np.errstate(invalid="ignore"):
                removed[i, :nr] = (wb.r_val[i, :nr, 1] != 0.0) & (r_chi2[i, :nr] > chi2_max)
    return removed, removed.sum(axis=1).astype(np.int32)


def margin(wb, r_chi2, chi2_max):
    """the smallest |chi2 / chi2_max - 1| over the batch's range rows with information != 0"""
    worst = np.inf
    for i in range(wb.B):
        nr = int(wb.counts[i, 1])
        live = wb.r_val[i, :nr, 1] != 0.0
        if live.any():
            worst = min(worst, float(np.abs(r_chi2[i, :nr][live] / chi2_max - 1.0).min()))
    return worst


def with_rows_zeroed(la, wb, removed):
    """a copy of wb whose flagged range rows have information 0.0 (what the prune leaves on the device)"""
    out = wb.copy()
    out.r_val[:, :, 1] = np.where(removed[:, :out.r_val.shape[1]] != 0, 0.0, out.r_val[:, :, 1])
    return out


def with_rows_deleted(la, wb, removed):
    """a copy of wb without the flagged range rows (the reference's level 1 as the oracle can express it: the edge is not in the graph)"""
    out = wb.copy()
    for i in range(wb.B):
        nr = int(wb.counts[i, 1])
        keep = [e for e in range(nr) if not removed[i, e]]
        out.r_idx[i] = 0; out.r_val[i] = 0.0
        out.r_idx[i, :len(keep)] = wb.r_idx[i, keep]; out.r_val[i, :len(keep)] = wb.r_val[i, keep]
        if out.r_off1 is not None:
            out.r_off1[i] = 0.0; out.r_off1[i, :len(keep)] = wb.r_off1[i, keep]
        out.counts[i, 1] = len(keep)
    return out
