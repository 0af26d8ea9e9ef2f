"""The graph families of tests/_graph_families.py on the CPU: the builders build what they say, relabel() moves a window without changing
it, and — the reason the GPU tests may hold window_lm_kernel to the oracle on these windows — the REFERENCE ALONE is stable on every one of
them: the oracle's 10-iteration solve of a window and of its relabelled copy (another elimination order of the same dense factorisation)
agree within a tenth of the GPU tolerance with equal LM trial counts, so no accept / reject decision of a case sits at a rounding edge
(DESIGN.md §3 records the figures this file prints)."""
import numpy as np
import pytest

import _graph_families as F
from _general_cov_inputs import window_pairs


def _norm(pairs):
    return sorted((min(p), max(p)) for p in pairs)


def test_builders():
    deg = lambda n, pairs: np.bincount(np.array(pairs).ravel(), minlength=n).tolist()
    assert deg(7, F.ring(7)) == [2] * 7 and len(F.ring(7)) == 7
    assert len(F.grid(3, 5)) == 3 * 4 + 2 * 5 and sorted(deg(15, F.grid(3, 5))) == [2] * 4 + [3] * 8 + [4] * 3
    assert len(F.clique(6)) == 15 and deg(6, F.clique(6)) == [5] * 6
    t = F.random_tree(np.random.default_rng(3), 25)
    assert len(t) == 24 and all(u < v for u, v in t) and sorted(v for _, v in t) == list(range(1, 25))
    cc = F.chain_with_clique(9, 4)
    assert len(set(_norm(cc))) == len(cc) == 5 + 6 and deg(9, cc) == [1, 2, 2, 2, 2, 4, 3, 3, 3]
    co = F.components(11)
    assert deg(11, co) == [1, 2, 2, 2, 1] + [2] * 6 and not any(u < 5 <= v for u, v in _norm(co))
    assert deg(8, F.ladder(4)) == [2, 2, 3, 3, 3, 3, 2, 2]
    b = F.banded_with_long_links(30, ((7, 5, 0), (12, 11, 3)))
    assert _norm(b) == sorted(F.chain(30) + [(0, 7), (5, 12), (10, 17), (15, 22), (20, 27), (3, 15), (14, 26)])
    a = F.arrowhead_with_pendant(5, 3)
    assert deg(9, a) == [4, 5, 5, 5, 4, 6, 5, 5, 1]
    for pairs in (cc, co, b, a, F.grid(3, 5), F.ladder(4)):
        assert len(set(_norm(pairs))) == len(pairs) and all(u != v for u, v in pairs)


def test_fill_graph_and_relabel(built):
    from localization_amd.window import WindowBatch
    pairs = F.grid(3, 4)
    for six in (True, False):
        wb = WindowBatch(2, 14, 80, 14, 10)
        F.fill_graph(wb, 1, np.random.default_rng(1), 12, pairs, six, doubled=(2, 5))
        nv, nr, npr, ns = (int(x) for x in wb.counts[1])
        assert (nv, npr, ns) == (12, 12 if six else 0, 6 if six else 0) and nr == 48 + len(pairs) - ns + 2
        assert (wb.counts[0] == 0).all()
        assert (np.bincount(wb.r_idx[1, :nr, 0][wb.r_idx[1, :nr, 1] < 0], minlength=12) == 4).all()     # every pose: four anchors
        assert _norm(set(_norm(window_pairs(wb, 1)))) == _norm(pairs) and F.shared_edges(wb, 1) == 4
        assert (wb.s_idx[1, :ns, 2] == 1).all() and six == bool((wb.r_val[1, :48, 2:] != 0).any())
        before = {n: getattr(wb, n).copy() for n in wb.TABLES}
        perm = np.random.default_rng(2).permutation(12)
        F.relabel(wb, 1, perm)
        for n in ("counts", "r_val", "p_val", "s_val"):
            assert np.array_equal(getattr(wb, n), before[n])
        assert np.array_equal(wb.poses[1, perm], before["poses"][1, :12]) and np.array_equal(wb.poses[1, 12:], before["poses"][1, 12:])
        assert np.array_equal(wb.r_idx[1, :nr, 0], perm[before["r_idx"][1, :nr, 0]])
        anchor = before["r_idx"][1, :nr, 1] < 0
        assert np.array_equal(wb.r_idx[1, :nr, 1][anchor], before["r_idx"][1, :nr, 1][anchor])
        assert np.array_equal(wb.r_idx[1, :nr, 1][~anchor], perm[before["r_idx"][1, :nr, 1][~anchor]])
        assert np.array_equal(wb.p_idx[1, :npr], perm[before["p_idx"][1, :npr]])
        assert np.array_equal(wb.s_idx[1, :ns, :2], perm[before["s_idx"][1, :ns, :2]]) and np.array_equal(wb.s_idx[1, :, 2:], before["s_idx"][1, :, 2:])
        F.relabel(wb, 1, np.argsort(perm))
        for n, a in before.items():
            assert np.array_equal(getattr(wb, n), a), n


def test_batches_are_what_they_say(built):
    for name, (six, bw, _, windows) in F.BATCHES.items():
        wb = F.build_batch(name)
        caps = F.batch_caps(name)
        assert tuple(int(x) for x in wb.counts.max(axis=0)) == caps[:4]
        wr = F.relabelled_batch(name)
        for i in range(wb.B):
            nv, pairs = F.window_spec(name, i)
            assert nv == wb.counts[i, 0] and _norm(set(_norm(window_pairs(wb, i)))) == _norm(pairs), (name, i)
            assert max(abs(u - v) for u, v in window_pairs(wb, i)) <= caps[4] and max(abs(u - v) for u, v in window_pairs(wr, i)) <= caps[4]
            perm = F.batch_perms(name)[i]
            assert _norm(set(_norm(window_pairs(wr, i)))) == _norm((perm[u], perm[v]) for u, v in pairs)
            assert six or (wb.counts[i, 2:] == 0).all()
        assert np.array_equal(F.build_batch(name).poses, wb.poses)                     # the same bits every time


@pytest.mark.parametrize("name", list(F.BATCHES))
def test_reference_is_stable_under_relabelling(built, name):
    for mode in F.batch_modes(name):
        tol_pose, tol_chi = F.TOL[mode]
        a, b = F.oracle_solution(name, mode), F.oracle_solution(name, mode, relabelled=True)
        worst_p = worst_c = 0.0
        for i, perm in enumerate(F.batch_perms(name)):
            (pa, ca, ia, ta), (pb, cb, ib, tb) = a[i], b[i]
            assert np.isfinite(pa).all() and ia == ib == 10 and ta == tb, (name, mode, i, ia, ib, ta, tb)
            worst_p = max(worst_p, np.abs(pa - pb[perm]).max())
            worst_c = max(worst_c, abs(ca - cb) / max(1.0, abs(ca)))
        print(f"reference stability {name:10s} {mode:8s}: poses {worst_p:.1e} (limit {tol_pose / 10:.0e}), chi2 {worst_c:.1e} relative (limit {tol_chi / 10:.0e})")
        assert worst_p < tol_pose / 10 and worst_c < tol_chi / 10, (name, mode, worst_p, worst_c)
