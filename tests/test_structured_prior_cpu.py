"""The inputs of tests/test_gpu_structured_prior.py are regular BY THE REFERENCE ALONE (the CPU oracle and numpy; no GPU): at the
oracle-solved poses every LDL^T pivot of H_kept is above 1e-9 of its diagonal entry, the oracle's ten-iteration solve is finite on every
case — the rank-1 and the all-zero matrices included —, and no window of a covariance case leaves the comparison but the one built to be
singular, which the pivot rule (1e-11) does refuse.  And no window amplifies the noise of the numeric Jacobians: the oracle's own two modes
end within 1e-6 m of each other."""
import functools

import numpy as np
import pytest

import _dense_prior_ref as D
import _structured_prior_cases as S


@pytest.fixture(scope="module")
def la():
    import localization_amd as la   # (host-side arrays only: no device is opened)
    return la


@functools.lru_cache(maxsize=None)
def _oracle(name, jac):
    import localization_amd as W
    from oracle import oracle as O
    wb = S.case_batch(W, name)
    mode = O.JAC_ANALYTIC if jac == "analytic" else O.JAC_NUMERIC_G2O
    for i in range(wb.B):
        nv = int(wb.counts[i, 0])
        wb.poses[i, :nv], _, _ = D.oracle_window(wb, i, S.ANCH, 10, mode)
    return wb, mode


@pytest.mark.parametrize("jac", ["analytic", "numeric"])
@pytest.mark.parametrize("name", list(S.CASES))
def test_cases_are_regular_at_the_oracles_poses(la, name, jac):
    wb, mode = _oracle(name, jac)
    assert np.isfinite(wb.poses).all()
    worst = np.inf
    for i in range(wb.B):
        nv = int(wb.counts[i, 0])
        assert np.array_equal(wb.poses[i, :nv, :9], np.broadcast_to(np.eye(3).reshape(9), (nv, 9)))   # translation-only: the rotations never move
        _, mask, H = D.covariance_ref(wb, i, S.ANCH, mode)
        assert (mask == 0b111000).all(), (i, mask)
        keep = np.diag(H) != 0.0
        piv = D.ldl_pivots(H[np.ix_(keep, keep)])
        if i in S.SINGULAR.get(name, ()):
            assert len(piv) < keep.sum() or piv.min() <= D.REL_PIVOT, (i, piv.min())
            continue
        assert len(piv) == keep.sum() and piv.min() > 1e-9, (name, i, piv.min())
        worst = min(worst, piv.min())
    print(f"structured prior inputs {name} {jac}: smallest relative LDL^T pivot {worst:.3e}")


@pytest.mark.parametrize("name", list(S.CASES))
def test_numeric_mode_noise_is_not_amplified(la, name):
    """the oracle's numeric and analytic solves of every window end within NUMERIC_GAP of each other (tests/_structured_prior_cases.py says why)"""
    a, _ = _oracle(name, "analytic")
    n, _ = _oracle(name, "numeric")
    gap = np.abs(a.poses - n.poses).max(axis=(1, 2))
    print(f"structured prior inputs {name}: oracle numeric against analytic, per window {gap}")
    assert (gap <= S.NUMERIC_GAP).all(), gap


def test_every_prior_matrix_is_a_psd_translation_block_and_the_ranks_are_all_there(la):
    ranks = set()
    for name in S.CASES:
        wb = S.case_batch(la, name)
        assert np.isnan(wb.p_val[:, :, 12:]).all()
        for i in range(wb.B):
            for e in range(int(wb.counts[i, 2])):
                W = wb.p_info[i, e].reshape(6, 6)
                assert np.array_equal(W, W.T) and not W[3:].any() and not W[:, 3:].any()
                ev = np.linalg.eigvalsh(W[:3, :3])
                assert ev.min() >= -1e-13 * max(ev.max(), 1.0)
                ranks.add(int((ev > 1e-9 * max(ev.max(), 1e-300)).sum()) if ev.max() > 0 else 0)
    assert ranks == {0, 1, 2, 3}
    assert sorted(S.COV_CASES) == sorted(["T2", "T6", "T10", "T64", "T40x2"]) and S.SINGULAR == {"singular": (3,)}
