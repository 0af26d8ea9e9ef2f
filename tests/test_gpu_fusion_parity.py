"""GPU parity of the fusion snapshot kernel (BASELINE config 3: 6-DoF, antenna lever arm, IMU rotation prior) vs the
oracle's general graph.  fp64, analytic Jacobians on both sides for the tight comparison; vs the g2o-faithful numeric
oracle with the looser bound (see tests/test_gpu_snapshot_parity.py for the reasoning behind the numbers)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _run(B, K, seed, iters=10, gate=3.0, **kw):
    import localization_amd as la
    from localization_amd.synthetic import make_fusion_stream
    s = make_fusion_stream(B, K, seed=seed, **kw)
    f = la.FusionSolver(s["anchors"], B, antenna_offset=s["offset"], maximum_iteration=iters, distance_outlier=gate, jacobian="analytic")
    f.set_poses(s["init"])
    pose, chi2, trials = f.solve(s["dist"], s["err"], s["imu"])
    last = f.get_poses()
    ms = f.last_kernel_ms()
    f.close()
    return s, pose, chi2, trials, last, ms


def _oracle(s, mode, iters=10, gate=3.0):
    from oracle import oracle as O
    return O.fusion_batch(s["anchors"], s["offset"], s["dist"], s["err"], s["imu"], s["init"], iterations=iters, gate=gate,
                          jac_mode=O.JAC_ANALYTIC if mode == "analytic" else O.JAC_NUMERIC_G2O)


def test_fusion_matches_oracle(gpu):
    s, pose, chi2, trials, last, ms = _run(1024 + 19, 4, seed=2)
    rp, rc, rt, rlast = _oracle(s, "analytic")
    d = np.abs(pose - rp)
    assert np.isfinite(pose).all()
    assert d[:, :3].max() < 1e-7 and np.median(d[:, :3]) < 1e-9, (d[:, :3].max(), np.median(d[:, :3]))
    assert d[:, 3:].max() < 1e-7                      # quaternion components
    assert np.abs(last - rlast).max() < 1e-7
    assert np.abs(chi2 - rc).max() <= 1e-6 * max(1.0, np.abs(rc).max())
    assert (trials != rt).mean() < 0.05


def test_fusion_vs_g2o_numeric_oracle(gpu):
    s, pose, chi2, trials, last, ms = _run(2048, 3, seed=4)
    rp, rc, rt, _ = _oracle(s, "numeric")
    d = np.abs(pose - rp).max(axis=1)
    assert np.median(d) < 1e-7 and np.quantile(d, 0.999) < 1e-5 and d.max() < 1e-3


def test_fusion_zero_lever_arm_reduces_to_snapshot(gpu):
    """With o = 0 the rotation decouples from the ranges (SURVEY §8(a) note): the rotation stays at the IMU's and, AT
    CONVERGENCE, positions equal the 3-DoF snapshot kernel's.  (Iterates differ: g2o's lambda_0 = 1e-5 * max diag(H) sees
    the prior's 2e5 rotation diagonal, so the 6-DoF problem is damped ~80x harder than the 3-DoF one.)"""
    import localization_amd as la
    from localization_amd.synthetic import make_fusion_stream
    B, K = 777, 3
    s = make_fusion_stream(B, K, seed=6, offset=(0.0, 0.0, 0.0))
    f = la.FusionSolver(s["anchors"], B, antenna_offset=(0, 0, 0), maximum_iteration=80, distance_outlier=3.0, jacobian="analytic")
    f.set_poses(s["init"])
    pose, chi2, trials = f.solve(s["dist"], s["err"], s["imu"])
    f.close()
    snap = la.SnapshotSolver(s["anchors"], B, maximum_iteration=80, distance_outlier=3.0, jacobian="analytic")
    snap.set_positions(s["init"][:3])
    spos, schi, _ = snap.solve(s["dist"], s["err"])
    snap.close()
    dd = np.abs(pose[:, :3] - spos).max(axis=1)
    assert np.quantile(dd, 0.99) < 1e-5, np.quantile(dd, [0.5, 0.9, 0.99, 1.0])   # (a few NLOS-laden tags converge slowly)
    q = pose[:, 3:7].transpose(0, 2, 1)
    qi = s["imu"][:, :, :4] * np.sign(s["imu"][:, :, 3:4])
    assert np.abs(q - qi).max() < 1e-9


def test_fusion_accuracy_and_properties(gpu):
    s, pose, chi2, trials, last, ms = _run(8192, 6, seed=8)
    e = np.sqrt(((pose[-1, :3] - s["truth_t"][-1]) ** 2).sum(axis=0))
    assert np.median(e) < 0.1 and (e > 0.5).mean() < 0.02
    s2, pose2, chi22, _, _, _ = _run(8192, 6, seed=8)
    assert np.array_equal(pose, pose2) and np.array_equal(chi2, chi22)          # deterministic
    from scipy.spatial.transform import Rotation
    dq = (Rotation.from_quat(pose[-1, 3:7].T).inv() * Rotation.from_quat(s["truth_q"][-1])).magnitude()
    assert np.median(dq) < 0.02


@pytest.mark.parametrize("B,K,M", [(777, 5, 8), (65536, 6, 8), (2048, 4, 6)])
def test_fusion_pipelined_host_path_equals_the_staged_one(gpu, B, K, M):
    """loc_fusion_solve_host_kmb (natural [K][M][B] layout, tiles packed on the GPU, chunked three-stream pipeline) is
    bit-identical to loc_fusion_solve_host on host-packed tiles, incl. an anchor count that needs padding."""
    import localization_amd as la
    from localization_amd.synthetic import make_fusion_stream
    s = make_fusion_stream(B, K, seed=9)
    anchors = s["anchors"][:M]
    dist, err = s["dist"][:, :M], s["err"][:, :M]
    a = la.FusionSolver(anchors, B, antenna_offset=s["offset"], maximum_iteration=10, distance_outlier=3.0, jacobian="analytic")
    a.set_poses(s["init"])
    ref = a.solve(dist, err, s["imu"])
    b = la.FusionSolver(anchors, B, antenna_offset=s["offset"], maximum_iteration=10, distance_outlier=3.0, jacobian="analytic")
    b.set_poses(s["init"])
    got = b.solve_stream(dist, err, s["imu"])
    for x, y in zip(ref, got):
        assert np.array_equal(x, y)
    assert np.array_equal(a.get_poses(), b.get_poses())
    a.close(); b.close()


def test_fusion_pipelined_host_path_regrows_its_buffers_on_one_handle(gpu):
    """One handle, loc_fusion_solve_host_kmb with 2 epochs, then 5 (every staging buffer is freed and allocated again; with
    covariances, whose staging is first allocated on a handle that already holds the solve's), then 3 (nothing regrows), then the
    staged loc_fusion_solve_host: each call bit-identical to the same call on a fresh handle.  6 anchors: padded tiles."""
    import localization_amd as la
    from localization_amd.synthetic import make_fusion_stream
    B, M = 777, 6
    s = make_fusion_stream(B, 5, seed=9)
    dist, err = s["dist"][:, :M], s["err"][:, :M]

    def solver():
        return la.FusionSolver(s["anchors"][:M], B, antenna_offset=s["offset"], maximum_iteration=10, distance_outlier=3.0, jacobian="analytic")

    def call(f, K, covariance):
        f.set_poses(s["init"])
        return f.solve_stream(dist[:K], err[:K], s["imu"][:K], covariance=covariance) if K else f.solve(dist, err, s["imu"])

    used = solver()
    for K, covariance in ((2, False), (5, True), (3, False), (0, False)):   # (0: the staged path, all epochs)
        fresh = solver()
        got, want = call(used, K, covariance), call(fresh, K, covariance)
        assert len(got) == (6 if covariance else 3)
        for i, (x, y) in enumerate(zip(got, want)):
            assert np.array_equal(x, y, equal_nan=(i == 3)), (K, covariance, i)   # (i == 3: a singular update's covariance is NaN on both)
        assert np.array_equal(used.get_poses(), fresh.get_poses())
        fresh.close()
    used.close()


@pytest.mark.parametrize("offset", [(0.1, 0.0, -0.05), (1.5, 0.5, -0.8)])
def test_fusion_numeric_mode_matches_numeric_oracle(gpu, offset):
    """The reference's configuration on both sides (g2o's central differences).  The short lever arm takes the perturbed norms from the
    central one (sqrt_ieee_near_c); a lever arm of more than a metre moves the antenna point by more than the 2e-9 m that shortcut is
    proven for (a rotation perturbation of 2e-9 rad times the arm), so the kernel takes the full IEEE square roots there."""
    import localization_amd as la
    from localization_amd.synthetic import make_fusion_stream
    s = make_fusion_stream(1024, 3, seed=9, offset=offset)
    f = la.FusionSolver(s["anchors"], 1024, antenna_offset=s["offset"], maximum_iteration=10, distance_outlier=3.0, jacobian="numeric")
    f.set_poses(s["init"])
    pose, chi2, trials = f.solve(s["dist"], s["err"], s["imu"])
    f.close()
    rp, rc, rt, _ = _oracle(s, "numeric")
    d = np.abs(pose - rp).max(axis=1)
    assert np.isfinite(pose).all()
    assert np.median(d) < 1e-7 and np.quantile(d, 0.999) < 1e-5 and d.max() < 1e-3, (np.median(d), np.quantile(d, 0.999), d.max())
