"""bench.py's JSON line on the GPU box, at small sizes: the headline is the reference's configuration (numeric Jacobians) with a
same-mode cpu_baseline (--full); for N > 1 (rehearsed with two gloo ranks sharing the one GPU) the --full line carries the §8(e) reporting
collectives; a plain run prints the headline alone and --dump-outputs writes the same last-step outputs run after run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(extra, timeout=600):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    run = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + extra, capture_output=True, text=True, timeout=timeout, env=env)
    assert run.returncode == 0, run.stderr[-3000:]
    return json.loads(run.stdout.strip().splitlines()[-1])


def test_headline_is_the_reference_configuration(gpu):
    j = _run(["--full", "--batch", "4096", "--epochs", "16", "--steps", "3", "--warmup", "1", "--legs", "cfg2_analytic", "--cpu-tags", "256", "--cpu-epochs", "32"])
    assert j["config"]["jacobian"] == "numeric" and j["dtype"] == "f64" and j["n_gpus"] == 1
    assert j["roofline"]["bound"] == "hbm" and j["roofline"]["kernel"].endswith("numeric>") and 0 < j["roofline"]["frac"] < 1
    cb = j["cpu_baseline"]
    # numeric vs numeric: 1e-5 m per update, up to the rare update whose LM accept / reject decision the 1e-7 noise of the difference quotient flips
    assert cb["kind"] == "port" and cb["cores"] == 1 and cb["median_abs_diff_vs_gpu_m"] < 1e-7 and cb["max_abs_diff_vs_gpu_m"] < 1e-4
    assert cb["frac_updates_diff_gt_1e-5_m"] <= 1e-3
    leg = j["legs"]["cfg2_analytic"]
    assert leg["jacobian"] == "analytic" and j["value_fast_mode"] == leg["value"] and leg["max_abs_diff_vs_cpu_baseline_m"] < 1e-3
    assert j["collectives"]["ranks"] == 1


def test_two_rank_gloo_rehearsal_carries_the_reporting_collectives(gpu):
    j = _run(["--full", "--gpus", "2", "--dist-backend", "gloo", "--batch", "4096", "--epochs", "8", "--steps", "2", "--warmup", "1", "--legs", "none", "--no-cpu-baseline"])
    assert j["n_gpus"] == 2 and j["ranks_joined"] == 2
    c = j["collectives"]
    assert c["ranks"] == 2 and c["backend"].startswith("gloo") and c["all_gather"]["checksum_ok"] is True
    assert c["all_gather"]["bytes"] == 2 * 4 * 4096 * 8 and c["all_reduce"]["bytes"] == 32 and c["bytes"] == c["all_gather"]["bytes"] + 32
    v = c["all_reduce"]["values"]
    assert v[0] > 0 and v[1] >= 2 * 4096 * 8 * 2 * 1 and v[2] == 0     # sum chi2, sum LM trials over both ranks' timed epochs, no non-finite estimate


def test_plain_run_is_the_headline_alone_and_dumps_repeatable_outputs(gpu, tmp_path):
    small = ["--batch", "4096", "--epochs", "16", "--steps", "3", "--warmup", "1"]
    runs = []
    for k in range(2):
        d = tmp_path / f"out{k}"
        j = _run(small + ["--dump-outputs", str(d)])
        assert j["steps"] == 3 and j["ms_per_step"] > 0 and j["unit"] == "updates/s" and j["higher_is_better"] is True and j["dtype"] == "f64"
        assert j["value"] == pytest.approx(4096 * 16 / (j["ms_per_step"] * 1e-3), rel=1e-9)
        assert not {"legs", "cpu_baseline", "collectives", "other_jacobian_mode"} & set(j)
        runs.append({n: np.load(d / f"{n}.npy") for n in ("positions", "chi2", "lm_trials")})
    a, b = runs
    # an independent anchor: the same seeded epochs (the library's stream) solved directly, one launch per step
    import torch
    import localization_amd as la
    from localization_amd.synthetic import ANCHORS_8, make_snapshot_stream_torch
    s = make_snapshot_stream_torch(4096, 4 * 16, seed=0, device=gpu)
    solver = la.SnapshotSolver(ANCHORS_8, 4096, maximum_iteration=10, distance_outlier=1.0, jacobian="numeric", device=0)
    solver.set_positions(s["init"])
    pos = torch.empty((64, 3, 4096), dtype=torch.float64, device=gpu)
    chi2 = torch.empty((64, 4096), dtype=torch.float64, device=gpu)
    trials = torch.empty((64, 4096), dtype=torch.uint8, device=gpu)
    for i in range(4):
        sl = slice(16 * i, 16 * (i + 1))
        solver.solve_device(s["dist_tiles"][sl], s["err_tiles"][sl], pos[sl], chi2[sl], trials[sl])
    torch.cuda.synchronize()
    solver.close()
    assert np.array_equal(a["positions"], pos[48:].cpu().numpy()) and np.array_equal(a["chi2"], chi2[48:].cpu().numpy())
    assert np.array_equal(a["lm_trials"], trials[48:].cpu().numpy().astype(np.float32))
    assert a["positions"].shape == (16, 3, 4096) and a["positions"].dtype == np.float64
    assert a["chi2"].shape == (16, 4096) and a["chi2"].dtype == np.float64
    assert a["lm_trials"].shape == (16, 4096) and a["lm_trials"].dtype == np.float32
    assert np.isfinite(a["positions"]).all()
    for n in a:
        assert np.array_equal(a[n], b[n]), n


def test_stream_generated_in_chunks_gives_the_same_outputs(gpu, tmp_path):
    """A run longer than --resident-gib holds generates the stream chunk by chunk (here 2 + 2 + 2 steps of 6.4 MB): the same epochs,
    the same solver state carried across, so the same outputs bit for bit as one resident stream; --full still runs on top of it."""
    small = ["--batch", "4096", "--epochs", "16", "--steps", "5", "--warmup", "1"]
    one = _run(small + ["--dump-outputs", str(tmp_path / "one")])
    chunked = _run(small + ["--resident-gib", "0.0125", "--dump-outputs", str(tmp_path / "chunked")])
    assert one["steps"] == chunked["steps"] == 5 and chunked["roofline"]["launches_timed"] == 5
    for n in ("positions", "chi2", "lm_trials"):
        assert np.array_equal(np.load(tmp_path / "one" / f"{n}.npy"), np.load(tmp_path / "chunked" / f"{n}.npy")), n
    j = _run(small + ["--resident-gib", "0.0125", "--full", "--legs", "cfg2_analytic", "--cpu-tags", "256", "--cpu-epochs", "32"])
    cb = j["cpu_baseline"]
    assert cb["median_abs_diff_vs_gpu_m"] < 1e-7 and cb["max_abs_diff_vs_gpu_m"] < 1e-4
    assert j["legs"]["cfg2_analytic"]["max_abs_diff_vs_cpu_baseline_m"] < 1e-3 and j["collectives"]["ranks"] == 1
    assert j["mean_lm_trials_per_update"] > 0


def test_bench_stream_is_the_library_stream_on_the_device(gpu):
    """bench.py's SnapshotStream on the GPU at the headline batch: make_snapshot_stream_torch's numbers bit for bit, across its batch
    boundaries and next() splits."""
    import importlib.util
    import torch
    from localization_amd.synthetic import make_snapshot_stream_torch
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec); spec.loader.exec_module(bench)
    B, K = 65536, 75
    ref = make_snapshot_stream_torch(B, K, seed=3, device=gpu)
    s = bench.SnapshotStream(B, 3, gpu)
    parts = [s.next(k) for k in (1, 40, 34)]
    assert torch.equal(torch.cat([p[0] for p in parts]), ref["dist_tiles"]) and torch.equal(torch.cat([p[1] for p in parts]), ref["err_tiles"])
    assert torch.equal(s.p, ref["truth_last"])
