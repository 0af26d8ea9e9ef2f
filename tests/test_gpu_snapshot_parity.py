"""GPU parity: HIP snapshot kernel (through the C ABI) vs the CPU oracle on the same seeded inputs.

Tolerances (floating point, fp64 on both sides):
  * same algorithm (analytic vs analytic, numeric vs numeric): 1e-7 m on every estimate, 1e-9 m on the median.
    The bound is not round-off alone: near convergence g2o's gain ratio is decided by chi differences at the
    1e-13 level, so an accept/reject can flip between two correct implementations and move the iterate by the
    size of that (converged) step, ~1e-8 m.
  * numeric vs numeric (delta = 1e-9): 1e-5 m max / 1e-7 m median — derivative noise, see the test body.
  * analytic kernel vs the g2o-faithful numeric oracle (delta = 1e-9 central differences): 1e-5 m.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _run(gpu, B, K, seed, jac, lpi, gate=1.0, iters=10, M=8, anchors=None, init_offset=None, **kw):
    import localization_amd as la
    from localization_amd.synthetic import ANCHORS_8, make_snapshot_stream
    from oracle import oracle as O
    anchors = ANCHORS_8[:M] if anchors is None else anchors
    s = make_snapshot_stream(B, K, seed=seed, anchors=anchors, **kw)
    if init_offset is not None:
        s["init"] = s["init"] + np.asarray(init_offset, dtype=np.float64)[:, None]
    solver = la.SnapshotSolver(anchors, B, maximum_iteration=iters, distance_outlier=gate, jacobian=jac,
                               lanes_per_instance=lpi)
    solver.set_positions(s["init"])
    pos, chi2, trials = solver.solve(s["dist"], s["err"])
    last = solver.get_positions()
    solver.close()
    return s, pos, chi2, trials, last


def _oracle(s, jac, gate=1.0, iters=10):
    from oracle import oracle as O
    mode = O.JAC_ANALYTIC if jac == "analytic" else O.JAC_NUMERIC_G2O
    return O.snapshot_batch(s["anchors"], s["dist"], s["err"], s["init"], iterations=iters, gate=gate, jac_mode=mode)


@pytest.mark.parametrize("lpi", [1, 2, 4, 8])
@pytest.mark.parametrize("jac", ["analytic", "numeric"])
def test_snapshot_matches_oracle(gpu, lpi, jac):
    B, K = 2048 + 37, 4  # ragged batch: not a multiple of the wave or block size
    s, pos, chi2, trials, last = _run(gpu, B, K, seed=11, jac=jac, lpi=lpi)
    rp, rc, rt, rlast = _oracle(s, jac)
    d = np.abs(pos - rp)
    # numeric mode: the delta = 1e-9 difference quotient multiplies every last-bit difference of sqrt/FMA by 5e8,
    # i.e. derivative noise ~1e-7 relative on BOTH sides (two CPU builds of g2o would differ the same way).
    tol_max, tol_med = (1e-7, 1e-9) if jac == "analytic" else (1e-5, 1e-7)
    assert d.max() < tol_max, d.max()
    assert np.median(d) < tol_med
    assert np.abs(last - rlast).max() < tol_max
    assert np.abs(chi2 - rc).max() <= (1e-6 if jac == "analytic" else 1e-3) * max(1.0, np.abs(rc).max())
    # LM trial counts agree except where a gain ratio sat on the rounding edge
    assert (trials != rt).mean() < (0.02 if jac == "analytic" else 0.5)


def test_analytic_kernel_vs_g2o_numeric_oracle(gpu):
    s, pos, chi2, trials, last = _run(gpu, 4096, 3, seed=5, jac="analytic", lpi=2)
    rp, rc, rt, _ = _oracle(s, "numeric")
    d = np.abs(pos - rp).max(axis=1)  # [K, B]
    # analytic vs numeric-Jacobian agree to <= 1e-5 m AT CONVERGENCE.  The reference stops after a fixed
    # 10 iterations, converged or not (epoch 0 starts at the anchor centroid, un-gated, with NLOS ranges), and an
    # unconverged iterate depends on the Jacobian noise; the CPU oracle's own two modes differ by the same amounts.
    assert np.median(d) < 1e-7 and np.quantile(d, 0.999) < 1e-5 and d.max() < 1e-3
    # ... and at convergence (100 iterations on both sides) every tag agrees to 1e-5 m
    s2, pos2, _, _, _ = _run(gpu, 4096, 3, seed=5, jac="analytic", lpi=2, iters=100)
    rp2, _, _, _ = _oracle(s2, "numeric", iters=100)
    assert np.abs(pos2 - rp2).max() < 1e-5


@pytest.mark.parametrize("M", [3, 4, 5, 8, 12, 16])
def test_anchor_counts_and_padding(gpu, M):
    rng = np.random.default_rng(M)
    anchors = np.concatenate([rng.uniform(-4, 4, (M, 2)), rng.uniform(0, 3, (M, 1))], axis=1)
    # 3-5 random anchors leave many tags (near-)degenerate (mirror solutions across the anchor plane, rank-deficient H
    # held up only by lambda) where a 10-iteration LM path is chaotic in the last bit, so the indexing/padding logic is
    # checked after 2 iterations there; 8+ anchors run the full 10.
    iters = 10 if M >= 8 else 2
    # (the centroid of 3 anchors lies in their plane: an exact saddle between the two mirror solutions, where rounding
    # noise picks the side — start off-plane instead)
    s, pos, chi2, trials, last = _run(gpu, 777, 2, seed=M, jac="analytic", lpi=1, M=M, anchors=anchors, iters=iters,
                                      init_offset=(0.3, -0.2, 0.5))
    rp, rc, rt, _ = _oracle(s, "analytic", iters=iters)
    d = np.abs(pos - rp).max(axis=1)
    assert np.isfinite(pos).all() and np.isfinite(chi2).all()
    if M >= 8:
        assert d.max() < 1e-6
        assert np.abs(chi2 - rc).max() <= 1e-6 * max(1.0, np.abs(rc).max())
    else:
        assert np.quantile(d, 0.99) < 1e-6, np.quantile(d, [0.5, 0.9, 0.99, 1.0])


def test_gate_off_and_heavy_outliers(gpu):
    s, pos, chi2, trials, last = _run(gpu, 1500, 3, seed=3, jac="analytic", lpi=2, gate=0.0, outlier_frac=0.15)
    rp, rc, rt, _ = _oracle(s, "analytic", gate=0.0)
    assert np.abs(pos - rp).max() < 1e-6


def test_all_ranges_gated_or_invalid(gpu):
    """No usable range for a tag: estimate must stay put, chi2 = 0, no LM trial (g2o: '0 vertices to optimize')."""
    import localization_amd as la
    from localization_amd.synthetic import ANCHORS_8, make_snapshot_stream
    B, K = 256, 2
    s = make_snapshot_stream(B, K, seed=1)
    s["dist"][:, :, :64] += 50.0          # every range of tags 0..63 fails the 1 m gate
    s["err"][:, :, 64:128] = 0.0          # invalid sigma: slot unused
    s["dist"][:, :, 128:160] = np.nan
    s["init"][:, 160:] = s["truth"][0][:, 160:] + 0.05   # the ordinary tags start near the truth (gate is on at once)
    solver = la.SnapshotSolver(ANCHORS_8, B, maximum_iteration=10, distance_outlier=1.0, gate_warmup_epochs=0, jacobian="analytic")
    solver.set_positions(s["init"])
    pos, chi2, trials = solver.solve(s["dist"], s["err"])
    solver.close()
    for k in range(K):
        assert np.array_equal(pos[k][:, :160], s["init"][:, :160])
    assert (chi2[:, :160] == 0).all() and (trials[:, :160] == 0).all()
    from oracle import oracle as O
    rp, rc, rt, _ = O.snapshot_batch(s["anchors"], s["dist"], s["err"], s["init"], iterations=10, gate=1.0,
                                     jac_mode=O.JAC_ANALYTIC, gate_from_epoch=0)
    assert np.abs(pos - rp).max() < 1e-7
    assert np.isfinite(pos).all() and np.isfinite(chi2).all()


def test_noise_free_ranges_recover_truth(gpu):
    """Known answer: exact ranges -> exact position (to float32 range quantisation ~ 3e-7 m)."""
    s, pos, chi2, trials, last = _run(gpu, 512, 2, seed=9, jac="analytic", lpi=2, sigma=0.0, outlier_frac=0.0, iters=20)
    assert np.abs(pos - s["truth"]).max() < 5e-6
    assert chi2.max() < 1e-6


def test_full_size_properties(gpu):
    """BASELINE size (B = 65 536): size-independent properties instead of the (slow) oracle on everything:
    permutation equivariance over tags, determinism, epoch-split idempotence, and an oracle spot check."""
    import localization_amd as la
    from localization_amd.synthetic import ANCHORS_8, make_snapshot_stream
    B, K = 65536, 4
    s = make_snapshot_stream(B, K, seed=21)
    def run(dist, err, init, lpi=2, split=False):
        solver = la.SnapshotSolver(ANCHORS_8, B, maximum_iteration=10, distance_outlier=1.0, lanes_per_instance=lpi, jacobian="analytic")
        solver.set_positions(init)
        if split:
            outs = [solver.solve(dist[k:k + 1], err[k:k + 1]) for k in range(K)]
            pos = np.concatenate([o[0] for o in outs]); chi2 = np.concatenate([o[1] for o in outs])
        else:
            pos, chi2, _ = solver.solve(dist, err)
        solver.close()
        return pos, chi2
    pos, chi2 = run(s["dist"], s["err"], s["init"])
    pos2, chi22 = run(s["dist"], s["err"], s["init"])
    assert np.array_equal(pos, pos2) and np.array_equal(chi2, chi22)            # deterministic
    perm = np.random.default_rng(0).permutation(B)
    posp, chi2p = run(s["dist"][:, :, perm], s["err"][:, :, perm], s["init"][:, perm])
    assert np.array_equal(posp, pos[:, :, perm]) and np.array_equal(chi2p, chi2[:, perm])  # tags are independent
    poss, chi2s = run(s["dist"], s["err"], s["init"], split=True)
    assert np.array_equal(poss, pos)                                            # K epochs in one launch == K launches
    pos1, _ = run(s["dist"], s["err"], s["init"], lpi=1)
    assert np.abs(pos1 - pos).max() < 1e-7                                      # lane mapping does not matter
    from oracle import oracle as O
    idx = np.arange(0, B, 64)
    rp, rc, _, _ = O.snapshot_batch(s["anchors"], s["dist"][:, :, idx], s["err"][:, :, idx], s["init"][:, idx],
                                    iterations=10, gate=1.0, jac_mode=O.JAC_ANALYTIC)
    assert np.abs(pos[:, :, idx] - rp).max() < 1e-7
    # accuracy sanity vs ground truth (not a reference number): after warm-up the estimate tracks the walk
    # (a fraction of a percent of tags sit in the mirror minimum above the 2 m anchor box — same in the oracle)
    e = np.sqrt(((pos[-1] - s["truth"][-1]) ** 2).sum(axis=0))
    assert np.median(e) < 0.1 and (e > 0.5).mean() < 0.02, (np.median(e), (e > 0.5).mean())


def test_device_resident_path_and_timing(gpu):
    import torch
    import localization_amd as la
    from localization_amd.synthetic import ANCHORS_8, make_snapshot_stream_torch
    B, K = 8192, 8
    s = make_snapshot_stream_torch(B, K, seed=4, device=gpu)
    solver = la.SnapshotSolver(ANCHORS_8, B, maximum_iteration=10, jacobian="analytic")
    solver.set_positions(s["init"])
    out_pos, out_chi2, out_trials = solver.alloc_outputs(K)
    solver.timing_begin(4)
    solver.solve_device(s["dist_tiles"], s["err_tiles"], out_pos, out_chi2, out_trials)
    torch.cuda.synchronize()
    n, tot, avg = solver.timing_end()
    assert n == 1 and tot > 0
    host = la.SnapshotSolver(ANCHORS_8, B, maximum_iteration=10, jacobian="analytic")
    host.set_positions(s["init"])
    d = la.unpack_ranges(s["dist_tiles"].cpu().numpy(), 8); e = la.unpack_ranges(s["err_tiles"].cpu().numpy(), 8)
    pos, chi2, trials = host.solve(d, e)
    assert np.array_equal(pos, out_pos.cpu().numpy())
    e = ((out_pos[-1] - s["truth_last"]) ** 2).sum(dim=0).sqrt()
    assert float(e.median()) < 0.1 and float((e > 0.5).double().mean()) < 0.02
    solver.close(); host.close()


@pytest.mark.parametrize("B,K,M", [(1000, 7, 8), (65536, 9, 8), (4096, 5, 5)])
def test_pipelined_host_path_equals_the_staged_one(gpu, B, K, M):
    """loc_snapshot_solve_host_kmb (natural [K][M][B] layout, packed on the GPU, chunked three-stream pipeline, pinned or
    pageable buffers) returns bit-identical positions, chi2 and trial counts to loc_snapshot_solve_host on host-packed
    tiles — including the warm-up epoch's un-gated solve when a chunk boundary falls after it, a ragged last chunk and
    an anchor count that needs padding."""
    import localization_amd as la
    from localization_amd.synthetic import ANCHORS_8, make_snapshot_stream
    s = make_snapshot_stream(B, K, seed=3)
    anchors = ANCHORS_8[:M]
    dist, err = s["dist"][:, :M], s["err"][:, :M]
    a = la.SnapshotSolver(anchors, B, maximum_iteration=10, distance_outlier=1.0, jacobian="analytic")
    a.set_positions(s["init"])
    ref = a.solve(dist, err)
    b = la.SnapshotSolver(anchors, B, maximum_iteration=10, distance_outlier=1.0, jacobian="analytic")
    b.set_positions(s["init"])
    got = b.solve_stream(dist, err)
    for x, y in zip(ref, got):
        assert np.array_equal(x, y)
    assert np.array_equal(a.get_positions(), b.get_positions())
    pd = b.pinned(dist.shape, np.float32); pe = b.pinned(err.shape, np.float32)
    pd[:] = dist; pe[:] = err
    b.set_positions(s["init"])
    got2 = b.solve_stream(pd, pe, (b.pinned((K, 3, B), np.float64), b.pinned((K, B), np.float64), b.pinned((K, B), np.uint8)))
    for x, y in zip(ref, got2):
        assert np.array_equal(x, y)
    a.close(); b.close()


def test_pipelined_host_path_regrows_its_buffers_on_one_handle(gpu):
    """One handle, loc_snapshot_solve_host_kmb with 2 epochs, then 5 (every staging buffer is freed and allocated again; with
    covariances, whose staging is first allocated on a handle that already holds the solve's), then 3 (nothing regrows), then the
    staged loc_snapshot_solve_host: each call bit-identical to the same call on a fresh handle.  5 anchors: padded tiles."""
    import localization_amd as la
    from localization_amd.synthetic import ANCHORS_8, make_snapshot_stream
    B, M = 1000, 5
    s = make_snapshot_stream(B, 5, seed=3)
    dist, err = s["dist"][:, :M], s["err"][:, :M]

    def solver():
        return la.SnapshotSolver(ANCHORS_8[:M], B, maximum_iteration=10, distance_outlier=1.0, jacobian="analytic")

    def call(sv, K, covariance):
        sv.set_positions(s["init"])
        return sv.solve_stream(dist[:K], err[:K], covariance=covariance) if K else sv.solve(dist, err)

    used = solver()
    for K, covariance in ((2, False), (5, True), (3, False), (0, False)):   # (0: the staged path, all epochs)
        fresh = solver()
        got, want = call(used, K, covariance), call(fresh, K, covariance)
        assert len(got) == (6 if covariance else 3)
        for i, (x, y) in enumerate(zip(got, want)):
            assert np.array_equal(x, y, equal_nan=(i == 3)), (K, covariance, i)   # (i == 3: a singular update's covariance is NaN on both)
        assert np.array_equal(used.get_positions(), fresh.get_positions())
        fresh.close()
    used.close()


def test_degenerate_inputs_start_on_an_anchor_and_non_finite_ranges(gpu):
    """Collisions and bad data, as the domain has them: (1) the estimate starts exactly ON an anchor (r = 0 for that edge:
    the analytic Jacobian is 0/0, g2o's numeric one is finite) — both Jacobian modes stay finite and match the oracle;
    (2) NaN / +-Inf distances and zero / negative / NaN distance_err mark a slot invalid: it is skipped, never poisons
    the estimate, and GPU and oracle agree."""
    import localization_amd as la
    from localization_amd.synthetic import ANCHORS_8, make_snapshot_stream
    from oracle import oracle as O
    B, K = 64, 3
    s = make_snapshot_stream(B, K, seed=5)
    init = s["init"].copy()
    for b in range(B):
        init[:, b] = ANCHORS_8[b % 8]
    for jm, oj, tol in (("analytic", O.JAC_ANALYTIC, 1e-7), ("numeric", O.JAC_NUMERIC_G2O, 1e-5)):
        sol = la.SnapshotSolver(ANCHORS_8, B, maximum_iteration=10, distance_outlier=0.0, jacobian=jm)
        sol.set_positions(init)
        gp, gc, _ = sol.solve(s["dist"], s["err"])
        rp, rc, _, _ = O.snapshot_batch(ANCHORS_8, s["dist"], s["err"], init, iterations=10, gate=0.0, jac_mode=oj)
        assert np.isfinite(gp).all() and np.isfinite(gc).all() and np.isfinite(rp).all()
        assert np.abs(gp - rp).max() < tol
        sol.close()
    d = s["dist"].copy(); e = s["err"].copy()
    d[0, 0, :8] = np.nan; d[1, 1, :8] = np.inf; d[2, 5, :8] = -np.inf
    e[0, 2, :8] = 0.0; e[1, 3, :8] = -1.0; e[2, 4, :8] = np.nan
    sol = la.SnapshotSolver(ANCHORS_8, B, maximum_iteration=10, distance_outlier=1.0, jacobian="analytic")
    sol.set_positions(s["init"])
    gp, gc, _ = sol.solve(d, e)
    rp, rc, _, _ = O.snapshot_batch(ANCHORS_8, d, e, s["init"], iterations=10, gate=1.0, jac_mode=O.JAC_ANALYTIC, gate_from_epoch=1)
    assert np.isfinite(gp).all() and np.isfinite(gc).all()
    assert np.abs(gp - rp).max() < 1e-9 and np.abs(gc - rc).max() < 1e-9 * max(1.0, np.abs(rc).max())
    sol.close()


@pytest.mark.parametrize("lpi", [1, 4])
def test_robust_chi2_is_a_sum_of_logs_that_does_not_overflow(gpu, lpi):
    """g2o sums rho = log(1 + chi2_j) edge by edge; the kernels take ONE log of the product, which overflows once eight factors
    exceed 1e38 each (|e| / sigma > 1e19: distance_err = 1e-23 here).  The guarded kernel falls back to the edge-by-edge sum for such a
    wave and must follow the oracle's LM decisions; before the guard every trial scored inf and was rejected."""
    import localization_amd as la
    from localization_amd.synthetic import ANCHORS_8, make_snapshot_stream
    from oracle import oracle as O
    B, K = 64 + 5, 2
    s = make_snapshot_stream(B, K, seed=3)
    s["err"] = np.full_like(s["err"], 1e-23)
    s["err"][:, :, ::2] = 0.055          # every second tag keeps physical sigmas: both kinds share a wave
    solver = la.SnapshotSolver(ANCHORS_8, B, maximum_iteration=10, distance_outlier=0.0, jacobian="analytic", lanes_per_instance=lpi)
    solver.set_positions(s["init"])
    pos, chi2, trials = solver.solve(s["dist"], s["err"])
    solver.close()
    rp, rc, rt, _ = O.snapshot_batch(s["anchors"], s["dist"], s["err"], s["init"], iterations=10, gate=0.0, jac_mode=O.JAC_ANALYTIC)
    assert np.isfinite(pos).all() and np.isfinite(rp).all()
    # Without the guard every trial of such a tag scores inf and is rejected: ten rejections, Terminate, the estimate stays at the
    # initial guess (decimetres from the oracle's).  With it the tag follows the oracle; where both have converged, accept / reject
    # decisions are ties at the rounding level of a cost of ~800, so a few tags take another (equally valid) sequence of tiny steps.
    d = np.abs(pos - rp).max(axis=1)
    assert np.median(d[:, 1::2]) < 1e-9 and d[:, 1::2].max() < 1e-3, (np.median(d[:, 1::2]), d[:, 1::2].max())
    assert d[:, ::2].max() < 1e-7                                  # the physical tags sharing those waves are untouched
    assert (trials[:, 1::2] == rt[:, 1::2]).mean() > 0.4 and np.abs(np.abs(rp - s["init"][None]).max(axis=1)[:, 1::2]).min() > 1e-4
    assert np.abs(chi2 - rc).max() <= 1e-3 * np.abs(rc).max()
