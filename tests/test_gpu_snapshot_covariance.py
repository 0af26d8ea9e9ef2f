"""GPU checks of the per-update covariances of the snapshot and fusion solvers (snapshot_lm_kernel / fusion_lm_kernel with COV = true,
through loc_snapshot_solve_*_cov and loc_fusion_solve_*_cov) against the numpy reference of tests/_snapshot_covariance_ref.py, at the
estimates the solve returns.  Definition and tolerances: DESIGN.md §2 / §3."""
import numpy as np
import pytest

from localization_amd import _lib
from _snapshot_covariance_ref import fusion_reference, snapshot_reference

pytestmark = pytest.mark.gpu

LOC_OK, LOC_ERR_SINGULAR = 0, -6
# Frobenius norm of (GPU block - reference block) relative to the reference block's.  Numeric: 10x the largest value measured
# on an MI355X over every case of this file is 9.2e-6 (9.2e-7: fusion with a lever arm — the reference linearises at the rotation rebuilt
# from the returned quaternion, 1e-16 away from the kernel's matrix, and the rotation columns' central differences divide that by 2e-9),
# so the 1e-6 cap holds.  An ill-conditioned H amplifies the last-bit differences of two correct evaluations by its condition number
# kappa: a block whose reference H has kappa > TOL / KAPPA_EPS is held to KAPPA_EPS * kappa instead (first-order bound of an inverse).
TOL = {"analytic": 1e-8, "numeric": 1e-6}
KAPPA_EPS = 1e-15
# (M_PAD, lanes per tag) pairs snapshot_supported accepts
MAPPINGS = [(4, 1), (4, 2), (4, 4), (8, 1), (8, 2), (8, 4), (8, 8), (12, 1), (16, 1), (16, 2), (16, 4), (16, 8)]
ANCH16 = np.array([[3.0, -3.0, 0.0], [3.0, 3.0, 2.0], [-3.0, 3.0, 0.0], [-3.0, -3.0, 2.0],
                   [3.0, -3.0, 2.0], [3.0, 3.0, 0.0], [-3.0, 3.0, 2.0], [-3.0, -3.0, 0.0],
                   [0.0, -3.0, 1.0], [3.0, 0.0, 1.5], [0.0, 3.0, 0.5], [-3.0, 0.0, 1.2],
                   [1.5, -3.0, 2.0], [3.0, 1.5, 0.2], [-1.5, 3.0, 1.8], [-3.0, -1.5, 0.7]])


def _oracle_mode(jac):
    from oracle import oracle as O
    return O.JAC_ANALYTIC if jac == "analytic" else O.JAC_NUMERIC_G2O


def _snap_device(s, lpi, jac, covariance=True, iters=10, gate=1.0):
    """one solve_device launch over the whole stream; numpy outputs (pos, chi2, trials[, cov_packed, mask, status])"""
    import torch
    import localization_amd as la
    K, M, B = s["dist"].shape
    sv = la.SnapshotSolver(s["anchors"], B, maximum_iteration=iters, distance_outlier=gate, jacobian=jac, lanes_per_instance=lpi)
    sv.set_positions(s["init"])
    outs = sv.alloc_outputs(K, covariance=covariance)
    sv.solve_device(sv.to_device_tiles(s["dist"]), sv.to_device_tiles(s["err"]), *outs)
    torch.cuda.synchronize()
    res = tuple(x.cpu().numpy() for x in outs)
    sv.close()
    return res


def _fusion_device(s, jac, covariance=True, iters=10, gate=3.0):
    import torch
    import localization_amd as la
    from localization_amd.snapshot import pack_ranges
    K, M, B = s["dist"].shape
    f = la.FusionSolver(s["anchors"], B, antenna_offset=s["offset"], maximum_iteration=iters, distance_outlier=gate, jacobian=jac)
    f.set_poses(s["init"])
    dev = torch.device("cuda", 0)
    d = torch.from_numpy(pack_ranges(s["dist"])).to(dev); e = torch.from_numpy(pack_ranges(s["err"])).to(dev)
    imu = torch.from_numpy(np.ascontiguousarray(s["imu"])).to(dev)
    outs = f.alloc_outputs(K, covariance=covariance)
    f.solve_device(d, e, imu, *outs)
    torch.cuda.synchronize()
    res = tuple(x.cpu().numpy() for x in outs)
    f.close()
    return res


def _compare(gpu_full, gpu_mask, gpu_status, ref, ref_mask, ref_ok, tol, kappa=None):
    """every block: status and mask equal; singular blocks all NaN; the others exactly symmetric, PSD, within tol (relative Frobenius).
    Returns the largest relative difference."""
    assert np.array_equal(gpu_mask, ref_mask), np.argwhere(gpu_mask != ref_mask)[:5]
    assert np.array_equal(gpu_status == LOC_ERR_SINGULAR, ~ref_ok), np.argwhere((gpu_status == LOC_ERR_SINGULAR) != ~ref_ok)[:5]
    assert np.isin(gpu_status, (LOC_OK, LOC_ERR_SINGULAR)).all()
    sing = gpu_status == LOC_ERR_SINGULAR
    assert np.isnan(gpu_full[sing]).all()
    G, R = gpu_full[~sing], ref[~sing]
    assert np.isfinite(G).all()
    assert np.array_equal(G, np.swapaxes(G, -1, -2))
    ev = np.linalg.eigvalsh(G)
    assert (ev >= -1e-12 * np.abs(ev).max(axis=-1, keepdims=True)).all()
    rn = np.linalg.norm(R, axis=(-2, -1))
    zero = rn == 0.0
    assert not G[zero].any()
    rel = np.linalg.norm(G - R, axis=(-2, -1))[~zero] / rn[~zero]
    bound = np.full(rel.shape, tol) if kappa is None else np.maximum(tol, KAPPA_EPS * kappa[~sing][~zero])
    assert (rel <= bound).all(), (rel.max(), np.argmax(rel / bound))
    return float(rel.max()) if rel.size else 0.0


def _snapshot_stream(M, B, K, seed):
    from localization_amd.synthetic import make_snapshot_stream
    return make_snapshot_stream(B, K, seed=seed, anchors=ANCH16[:M])


@pytest.mark.parametrize("jac", ["analytic", "numeric"])
@pytest.mark.parametrize("M,lpi", MAPPINGS)
def test_snapshot_covariance_matches_reference(gpu, M, lpi, jac):
    B, K = 131, 3
    s = _snapshot_stream(M, B, K, seed=10 + M + lpi)
    pos, chi2, trials, cov, mask, status = _snap_device(s, lpi, jac)
    kappa = np.ones((K, B))
    ref, rmask, rok, nact = snapshot_reference(s["anchors"], s["dist"], s["err"], s["init"], pos, _oracle_mode(jac), kappa=kappa)
    worst = _compare(_lib.unpack_covariance(cov, 3), mask, status, ref, rmask, rok, TOL[jac], kappa)
    print(f"COVERR snapshot M={M} lpi={lpi} {jac}: max rel Frobenius {worst:.3e}, max kappa {kappa.max():.2e}")


@pytest.mark.parametrize("jac", ["analytic", "numeric"])
@pytest.mark.parametrize("lever", [True, False])
def test_fusion_covariance_matches_reference(gpu, jac, lever):
    import localization_amd as la
    from localization_amd.synthetic import make_fusion_stream
    B, K = 131, 3
    s = make_fusion_stream(B, K, seed=21 + lever, offset=(0.1, 0.0, -0.05) if lever else (0.0, 0.0, 0.0))
    f = la.FusionSolver(s["anchors"], B, antenna_offset=s["offset"], maximum_iteration=10, distance_outlier=3.0, jacobian=jac)
    f.set_poses(s["init"])
    pose, chi2, trials, cov, mask, status = f.solve_stream(s["dist"], s["err"], s["imu"], covariance=True)
    f.close()
    assert cov.shape == (K, B, 6, 6)
    kappa = np.ones((K, B))
    ref, rmask, rok, nact = fusion_reference(s["anchors"], s["offset"], s["dist"], s["err"], s["imu"], s["init"], pose, _oracle_mode(jac),
                                             kappa=kappa)
    worst = _compare(cov, mask, status, ref, rmask, rok, TOL[jac], kappa)
    print(f"COVERR fusion lever={lever} {jac}: max rel Frobenius {worst:.3e}, max kappa {kappa.max():.2e}")


def _inject(s, tags, epochs, anchors, delta=1.5):
    s = dict(s)
    d = s["dist"].copy()
    for b in tags:
        for k in epochs:
            for m in anchors(b):
                d[k, m, b] += np.float32(delta)
    s["dist"] = d
    return s


def test_gate_is_honoured(gpu):
    """Ranges the outlier gate rejects on the prior are not in H: the covariance matches the reference without them and differs
    measurably from one computed with every range (Cauchy alone leaves a 1.5 m outlier a small but visible weight)."""
    B, K = 128, 3
    s = _inject(_snapshot_stream(8, B, K, seed=5), range(1, B, 4), (1, 2), lambda b: (b % 8, (b + 3) % 8))
    pos, chi2, trials, cov, mask, status = _snap_device(s, 1, "analytic")
    full = _lib.unpack_covariance(cov, 3)
    mode = _oracle_mode("analytic")
    ref, rmask, rok, nact = snapshot_reference(s["anchors"], s["dist"], s["err"], s["init"], pos, mode)
    _compare(full, mask, status, ref, rmask, rok, TOL["analytic"])
    ref_all, _, _, nact_all = snapshot_reference(s["anchors"], s["dist"], s["err"], s["init"], pos, mode, use_gate=False)
    gated = nact < nact_all
    assert gated.sum() >= 60, gated.sum()   # (the 64 injected updates, and the stream's own NLOS ones)
    rel = np.linalg.norm(full - ref_all, axis=(-2, -1)) / np.linalg.norm(ref_all, axis=(-2, -1))
    assert rel[gated].min() > 1e-5, rel[gated].min()
    assert rel[~gated].max() <= TOL["analytic"]


def test_singular_update_is_isolated(gpu):
    """A tag whose gate leaves two anchors gets LOC_ERR_SINGULAR and NaN for that update; every other tag's outputs are bit-identical to
    the batch without that tag's outliers."""
    B, K, bad = 128, 3, 37
    clean = _snapshot_stream(8, B, K, seed=8)
    dirty = _inject(clean, [bad], [1], lambda b: range(2, 8))
    a = _snap_device(clean, 1, "analytic")
    d = _snap_device(dirty, 1, "analytic")
    cov, mask, status = d[3], d[4], d[5]
    assert status[1, bad] == LOC_ERR_SINGULAR and np.isnan(cov[1, :, bad]).all() and mask[1, bad] == 0
    assert (np.delete(status, bad, axis=-1) == LOC_OK).all()
    for x, y in zip(a, d):
        assert np.array_equal(np.delete(x, bad, axis=-1), np.delete(y, bad, axis=-1), equal_nan=True)


@pytest.mark.parametrize("jac", ["analytic", "numeric"])
def test_snapshot_solve_is_unchanged_on_the_device_path(gpu, jac):
    for M, lpi in [(8, 1), (16, 1), (16, 2), (16, 4), (16, 8), (4, 4), (12, 1)]:
        s = _snapshot_stream(M, 1000, 3, seed=30 + M)
        off = _snap_device(s, lpi, jac, covariance=False)
        on = _snap_device(s, lpi, jac, covariance=True)
        for x, y in zip(off, on[:3]):
            assert np.array_equal(x, y), (M, lpi)


def _pinned_copy(solver, x):
    p = solver.pinned(x.shape, x.dtype)
    p[...] = x
    return p


@pytest.mark.parametrize("lpi", [1, 2, 4, 8])
def test_snapshot_host_kmb_covariance_equals_the_device_path(gpu, lpi):
    """loc_snapshot_solve_host_kmb_cov over two pipeline chunks (page-locked buffers): the solve equals the plain host path's, the
    covariances equal one device launch's, bit for bit."""
    import localization_amd as la
    B, K = 65536, 6   # 8 anchors: 4 epochs per chunk
    s = _snapshot_stream(8, B, K, seed=12)
    dev = _snap_device(s, lpi, "numeric", iters=10)
    sv = la.SnapshotSolver(s["anchors"], B, maximum_iteration=10, distance_outlier=1.0, jacobian="numeric", lanes_per_instance=lpi)
    d, e = _pinned_copy(sv, s["dist"]), _pinned_copy(sv, s["err"])
    sv.set_positions(s["init"])
    plain = sv.solve_stream(d, e)
    out = (sv.pinned((K, 3, B), np.float64), sv.pinned((K, B), np.float64), sv.pinned((K, B), np.uint8),
           sv.pinned((K, 6, B), np.float64), sv.pinned((K, B), np.int32), sv.pinned((K, B), np.int32))
    sv.set_positions(s["init"])
    res = sv.solve_stream(d, e, out=out, covariance=True)
    try:   # (the page-locked outputs live until the solver is closed)
        for x, y, z in zip(plain, res[:3], dev[:3]):
            assert np.array_equal(x, y) and np.array_equal(y, z)
        assert np.array_equal(out[3], dev[3], equal_nan=True) and np.array_equal(res[4], dev[4]) and np.array_equal(res[5], dev[5])
        assert np.array_equal(res[3], _lib.unpack_covariance(dev[3], 3), equal_nan=True)
    finally:
        sv.close()


@pytest.mark.parametrize("jac", ["analytic", "numeric"])
def test_fusion_solve_is_unchanged_and_host_kmb_equals_device(gpu, jac):
    """fusion: cov on / off give the same solve on the device path; the pipelined host path over two chunks gives the device path's
    solve and covariances bit for bit."""
    import localization_amd as la
    from localization_amd.synthetic import make_fusion_stream
    B, K = 65536, 3   # 2 epochs per chunk
    s = make_fusion_stream(B, K, seed=40)
    off = _fusion_device(s, jac, covariance=False)
    on = _fusion_device(s, jac, covariance=True)
    for x, y in zip(off, on[:3]):
        assert np.array_equal(x, y)
    f = la.FusionSolver(s["anchors"], B, antenna_offset=s["offset"], maximum_iteration=10, distance_outlier=3.0, jacobian=jac)
    d, e, imu = _pinned_copy(f, s["dist"]), _pinned_copy(f, s["err"]), _pinned_copy(f, s["imu"])
    out = (f.pinned((K, 7, B), np.float64), f.pinned((K, B), np.float64), f.pinned((K, B), np.uint8),
           f.pinned((K, 21, B), np.float64), f.pinned((K, B), np.int32), f.pinned((K, B), np.int32))
    f.set_poses(s["init"])
    res = f.solve_stream(d, e, imu, covariance=True, out=out)
    f.set_poses(s["init"])
    plain = f.solve_stream(d, e, imu)
    try:   # (the page-locked outputs live until the solver is closed)
        for x, y, z in zip(plain, res[:3], off):
            assert np.array_equal(x, y) and np.array_equal(y, z)
        assert np.array_equal(out[3], on[3], equal_nan=True) and np.array_equal(res[4], on[4]) and np.array_equal(res[5], on[5])
    finally:
        f.close()


def test_python_surface(gpu):
    import torch
    import localization_amd as la
    from localization_amd.synthetic import make_fusion_stream
    B, K = 70, 2
    s = _snapshot_stream(8, B, K, seed=3)
    sv = la.SnapshotSolver(s["anchors"], B, maximum_iteration=10, jacobian="analytic")
    sv.set_positions(s["init"])
    plain = sv.solve_stream(s["dist"], s["err"])
    assert len(plain) == 3
    sv.set_positions(s["init"])
    pos, chi2, trials, cov, mask, status = sv.solve_stream(s["dist"], s["err"], covariance=True)
    assert pos.shape == (K, 3, B) and cov.shape == (K, B, 3, 3) and mask.shape == (K, B) and status.shape == (K, B)
    assert mask.dtype == np.int32 and status.dtype == np.int32 and (status == LOC_OK).all()
    assert np.array_equal(cov, np.swapaxes(cov, -1, -2)) and (np.diagonal(cov, axis1=-2, axis2=-1) > 0).all()
    assert all(np.array_equal(x, y) for x, y in zip(plain, (pos, chi2, trials)))
    outs = sv.alloc_outputs(K, covariance=True)
    assert len(outs) == 6 and tuple(outs[3].shape) == (K, 6, B) and outs[4].dtype == torch.int32
    assert len(sv.alloc_outputs(K)) == 3
    d, e = sv.to_device_tiles(s["dist"]), sv.to_device_tiles(s["err"])
    with pytest.raises(ValueError):
        sv.solve_device(d, e, *outs[:3], out_cov=outs[3])
    with pytest.raises(ValueError):
        sv.solve_device(d, e, *outs[:3], out_cov=outs[3], out_cov_mask=outs[4])
    sv.close()
    fs = make_fusion_stream(B, K, seed=3)
    f = la.FusionSolver(fs["anchors"], B, antenna_offset=fs["offset"], jacobian="analytic")
    f.set_poses(fs["init"])
    assert len(f.solve_stream(fs["dist"], fs["err"], fs["imu"])) == 3
    f.set_poses(fs["init"])
    pose, chi2, trials, cov6, mask6, status6 = f.solve_stream(fs["dist"], fs["err"], fs["imu"], covariance=True)
    assert pose.shape == (K, 7, B) and cov6.shape == (K, B, 6, 6) and mask6.shape == (K, B) and (status6 == LOC_OK).all()
    assert np.array_equal(cov6, np.swapaxes(cov6, -1, -2))
    fo = f.alloc_outputs(K, covariance=True)
    assert len(fo) == 6 and tuple(fo[3].shape) == (K, 21, B)
    from localization_amd.snapshot import pack_ranges
    dev = torch.device("cuda", 0)
    dt, et = torch.from_numpy(pack_ranges(fs["dist"])).to(dev), torch.from_numpy(pack_ranges(fs["err"])).to(dev)
    with pytest.raises(ValueError):
        f.solve_device(dt, et, torch.from_numpy(fs["imu"]).to(dev), *fo[:3], out_cov_status=fo[5])
    f.close()
