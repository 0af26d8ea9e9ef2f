"""The numeric snapshot pass takes ONE range vote per wave and pass (snapshot_kernel.hip: range_vote): a wave whose active lanes all
have every squared range in [1e-5, 1e300) runs the pass without the per-edge test, any other wave runs the pass that tests every edge.

Tags are independent, so what a tag computes must not depend on which of the two passes its wave-mates sent it through: the same
inputs with and without two off-range tags in the batch give every OTHER tag the same bits (no tolerance: view(int64)).  The two
off-range tags themselves are held to the oracle the way test_gpu_snapshot_parity.py holds its degenerate inputs (1e-5 m in numeric
mode, the same NaNs):
  * one tag starts ON anchor 2 with range 0 to it and the anchor's true ranges to the others: it stays there (the oracle leaves it
    within 6e-8 m of the anchor), so its wave votes for the tested pass in every pass of every epoch;
  * one tag has a NaN prior coordinate.
B = 96 is one full wave plus a half wave with dead lanes at one lane per tag; the off-range pair sits in the full wave (tags 5, 6) or in
the half-filled one (tags 70, 71), where dead lanes, and at the end of the launch an exhausted lane on an anchor, must not vote.
K = 1 and K = 2 are the edge cases of the kernel's two-epoch window.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B = 96
ON_ANCHOR = 2


@functools.lru_cache(maxsize=None)
def _stream(K):
    from localization_amd.synthetic import make_snapshot_stream
    s = make_snapshot_stream(B, K, seed=21)
    for v in s.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return s


def _solve(dist, err, init, lpi):
    import localization_amd as la
    from localization_amd.synthetic import ANCHORS_8
    solver = la.SnapshotSolver(ANCHORS_8, B, maximum_iteration=10, distance_outlier=1.0, jacobian="numeric", lanes_per_instance=lpi)
    solver.set_positions(init)
    pos, chi2, trials = solver.solve(dist, err)
    last = solver.get_positions()
    solver.close()
    return pos, chi2, trials, last


@functools.lru_cache(maxsize=None)
def _ordinary(K, lpi):
    """Run A: the stream as it is (every wave takes the pass without the test)."""
    s = _stream(K)
    return _solve(s["dist"], s["err"], s["init"], lpi)


def _with_off_range_pair(K, t_anchor, t_nan):
    from localization_amd.synthetic import ANCHORS_8
    s = _stream(K)
    dist, init = s["dist"].copy(), s["init"].copy()
    init[:, t_anchor] = ANCHORS_8[ON_ANCHOR]
    dist[:, :, t_anchor] = np.linalg.norm(ANCHORS_8 - ANCHORS_8[ON_ANCHOR], axis=1).astype(dist.dtype)[None, :]   # (0 to the anchor itself)
    init[0, t_nan] = np.nan
    return dist, s["err"], init


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def _check(K, lpi, t_anchor, t_nan):
    from localization_amd.synthetic import ANCHORS_8
    from oracle import oracle as O
    pos_a, chi_a, trials_a, last_a = _ordinary(K, lpi)
    dist, err, init = _with_off_range_pair(K, t_anchor, t_nan)
    pos_b, chi_b, trials_b, last_b = _solve(dist, err, init, lpi)

    others = np.ones(B, dtype=bool)
    others[[t_anchor, t_nan]] = False
    assert np.array_equal(_bits(pos_a)[:, :, others], _bits(pos_b)[:, :, others])
    assert np.array_equal(_bits(chi_a)[:, others], _bits(chi_b)[:, others])
    assert np.array_equal(trials_a[:, others], trials_b[:, others])
    assert np.array_equal(_bits(last_a)[:, others], _bits(last_b)[:, others])

    rp, rc, _, _ = O.snapshot_batch(ANCHORS_8, dist, err, init, iterations=10, gate=1.0, jac_mode=O.JAC_NUMERIC_G2O)
    # the tag on the anchor: finite, the oracle's estimate, and still on the anchor (so it was off range in every pass)
    assert np.isfinite(pos_b[:, :, t_anchor]).all() and np.isfinite(chi_b[:, t_anchor]).all()
    assert np.abs(pos_b[:, :, t_anchor] - rp[:, :, t_anchor]).max() < 1e-5
    assert np.abs(pos_b[:, :, t_anchor] - ANCHORS_8[ON_ANCHOR][None, :]).max() < 1e-3
    # the tag with the NaN prior: NaN where the oracle has NaN, the oracle's numbers elsewhere
    assert np.array_equal(np.isnan(pos_b[:, :, t_nan]), np.isnan(rp[:, :, t_nan]))
    assert np.isnan(pos_b[:, 0, t_nan]).all()
    assert np.abs(pos_b[:, 1:, t_nan] - rp[:, 1:, t_nan]).max() < 1e-5
    assert np.array_equal(np.isnan(chi_b[:, t_nan]), np.isnan(rc[:, t_nan]))


@pytest.mark.parametrize("lpi", [1, 2])
def test_off_range_tags_in_a_full_wave_leave_their_wave_mates_bits_alone(gpu, lpi):
    _check(6, lpi, 5, 6)


@pytest.mark.parametrize("lpi", [1, 2])
def test_off_range_tags_in_the_half_filled_wave(gpu, lpi):
    _check(6, lpi, 70, 71)


@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("lpi", [1, 2])
def test_window_edge_cases_one_and_two_epochs(gpu, lpi, K):
    _check(K, lpi, 5, 6)
