"""CPU checks of the marginal prior of a dropped pose (loc_window_marginal_prior_host), on the oracle and numpy alone, and of
the host check that stands between a caller's drop slots and the kernel (tests/host/marginal_drop_driver.cpp: window_structure.cpp compiled
from source with g++ under AddressSanitizer + UBSan, its own main, no HIP call).

* the numpy statement of the definition (tests/_dense_prior_ref.marginal_ref) against a dense elimination by least squares;
* the inputs of tests/test_gpu_marginal_prior.py are regular BY THE REFERENCE ALONE, at the oracle-solved poses: every LDL^T pivot of H^r_dd
  above 1e-9 of its diagonal entry, kept eigenvalues of Lambda >= 1e-6 lambda_max, dropped ones <= 1e-13 lambda_max;
* the one-drop property on the oracle alone, on the GPU tests' own inputs: with the marginal prior the kept poses move less than 1 / 100 of
  what the plain drop moves them when the shortened window is solved again;
* the host check: drop slots out of range, two neighbours, a neighbour through a doubled edge, ragged counts, poisoned unused slots."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import _dense_prior_ref as D
import _fixed_lag as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "localization_amd", "csrc")
I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31


@functools.lru_cache(maxsize=None)
def _oracle_solved(name, jac):
    """a parity case of tests/_fixed_lag.py at the oracle-solved poses (shared, never modified), its drop slots"""
    import localization_amd as la
    from oracle import oracle as O
    wb, drop = F.case_batch(la, name)
    mode = O.JAC_ANALYTIC if jac == "analytic" else O.JAC_NUMERIC_G2O
    for i in range(wb.B):
        nv = int(wb.counts[i, 0])
        wb.poses[i, :nv] = D.oracle_window(wb, i, F.ANCH, 10, mode)[0]
    return wb, drop, mode


@pytest.mark.parametrize("jac", ["analytic", "numeric"])
@pytest.mark.parametrize("name", list(F.CASES))
def test_numpy_statement_against_a_dense_elimination(name, jac):
    wb, drop, mode = _oracle_solved(name, jac)
    seen = 0
    for i in range(wb.B):
        ref = D.marginal_ref(wb, i, F.ANCH, mode, int(drop[i]))
        if ref["slot"] < 0 or ref["status"] != 0:
            continue
        Lam, gamma = D.marginal_by_elimination(ref["H"], ref["g"])
        e_lam = np.linalg.norm(Lam - ref["Lam"]) / np.linalg.norm(Lam)
        e_gam = np.linalg.norm(gamma - ref["gamma"]) / ref["term"]
        print(f"{name} {jac} window {i}: Lambda {e_lam:.2e}, gamma {e_gam:.2e}")
        assert e_lam <= 1e-10 and e_gam <= 1e-10, (i, e_lam, e_gam)
        # the prior row stands for that quadratic: residual e0 at x_m, gradient Lambda e0 = gamma, Hessian Lambda
        info = ref["prior"][12:].reshape(6, 6)
        e0 = D.prior_residual(ref["prior"], wb.poses[i, ref["slot"]])
        assert np.abs(e0 - ref["shift"][:3]).max() <= 1e-15   # ((e0 - t_m) + t_m: half an ulp of a translation below 4 m)
        assert np.linalg.norm(info[:3, :3] @ e0 - gamma) <= 1e-9 * ref["term"]
        assert np.linalg.norm(info[:3, :3] - Lam) <= 1e-10 * np.linalg.norm(Lam)
        seen += 1
    assert seen or name in ("chain1",)


@pytest.mark.parametrize("jac", ["analytic", "numeric"])
@pytest.mark.parametrize("name", list(F.CASES))
def test_gpu_inputs_are_regular_by_the_reference_alone(name, jac):
    wb, drop, mode = _oracle_solved(name, jac)
    for i in range(wb.B):
        ref = D.marginal_ref(wb, i, F.ANCH, mode, int(drop[i]))
        spec = F.CASES[name][i]
        if spec.get("one_range"):
            assert ref["status"] == D.LOC_ERR_SINGULAR and ref["slot"] >= 0 and ref["pivots"].min() <= 1e-13, (i, ref["pivots"])
            continue
        assert ref["status"] == 0
        if ref["slot"] < 0:
            assert spec["T"] == 1 or spec.get("missing")
            continue
        lam = ref["eig"]
        kept = lam > D.REL_PIVOT * lam.max()
        print(f"{name} {jac} window {i}: pivots {ref['pivots']}, eigenvalues / max {lam / lam.max()}, rank {ref['rank']}")
        assert ref["pivots"].min() > 1e-9, (i, ref["pivots"])
        assert ref["rank"] >= 1 and (lam[kept] >= 1e-6 * lam.max()).all() and (np.abs(lam[~kept]) <= 1e-13 * lam.max()).all(), (i, lam)


def _movement(la, O, wb, mode, with_prior):
    """the largest movement of the kept poses when pose 0 of every (oracle-solved) window is dropped and the shortened window solved again"""
    W = int(wb.counts[0, 0])
    chains = wb.chains
    rows = np.stack([D.marginal_ref(wb, i, F.ANCH, mode, 0)["prior"] for i in range(wb.B)])
    slots = np.array([D.marginal_ref(wb, i, F.ANCH, mode, 0)["slot"] for i in range(wb.B)])
    short = la.WindowBatch(wb.B, *F.window_caps(W))
    for i, ch in enumerate(chains):
        F.add_chain_poses(short, i, ch, 1, W - 1, est=wb.poses[i, 1:W, 9:12])
        if with_prior:
            F.add_prior_row(short, i, 0, rows[i])
            assert slots[i] == 1
    moved = []
    for i in range(wb.B):
        after = D.oracle_window(short, i, F.ANCH, F.PROPERTY_ITERATIONS, mode)[0]
        moved.append(np.abs(after[:, 9:] - wb.poses[i, 1:W, 9:12]).max())
    return np.array(moved)


@pytest.mark.parametrize("jac", ["analytic", "numeric"])
def test_one_drop_property_on_the_oracle(jac):
    import localization_amd as la
    from oracle import oracle as O
    mode = O.JAC_ANALYTIC if jac == "analytic" else O.JAC_NUMERIC_G2O
    chains = [F.Chain(7900 + i, 6, 3 + i % 2) for i in range(8)]   # (the fixed-lag test's chains, first window)
    wb = F.first_window(la, chains, 6)
    for i in range(wb.B):
        wb.poses[i, :6] = D.oracle_window(wb, i, F.ANCH, F.PROPERTY_ITERATIONS, mode)[0]
    wb.chains = chains
    with_prior, plain = _movement(la, O, wb, mode, True), _movement(la, O, wb, mode, False)
    print(f"one drop {jac}: kept poses move {with_prior} m with the marginal prior, {plain} m with the plain drop")
    assert (with_prior < plain / 100).all(), (with_prior, plain)


# ---- the host check under AddressSanitizer + UBSan ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("marginal_drop_driver")
    cxx = shutil.which("g++")
    assert cxx is not None, "g++ is needed to build tests/host/marginal_drop_driver.cpp (the project's build() needs it as well)"
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    rocm = os.path.dirname(os.path.dirname(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")))
    src = [os.path.join(ROOT, "tests", "host", "marginal_drop_driver.cpp"), os.path.join(CSRC, "window_structure.cpp")]
    logs = []
    for extra in (["-static-libasan", "-static-libubsan"], []):   # (the runtimes as archives where the compiler has them)
        r = subprocess.run([cxx, "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), "-I", CSRC, "-pthread", *flags, *extra, *src,
                            "-o", str(d / "driver")], capture_output=True, text=True)
        logs.append(" ".join(extra) + ": " + r.stderr[-1500:])
        if r.returncode == 0:
            return str(d / "driver")
    raise AssertionError("\n".join(logs))


def _write(f, wb, drop, n_anchors, pinfo=None):
    """one batch in the driver's format, every table at exactly its capacity"""
    nv, nr, npr, ns = wb.caps
    np.array([nv, nr, npr, ns, max(nv - 1, 0), n_anchors, pinfo is not None, 0], dtype=np.int32).tofile(f)
    np.array([wb.B], dtype=np.int64).tofile(f)
    for a, cap in ((wb.poses, nv), (wb.counts, None), (wb.r_val, nr), (wb.p_val, npr), (wb.s_val, ns), (wb.r_idx, nr), (wb.p_idx, npr), (wb.s_idx, ns)):
        np.ascontiguousarray(a if cap is None else a[:, :cap]).tofile(f)
    np.asarray(drop, dtype=np.int32).tofile(f)
    if pinfo is not None:
        np.ascontiguousarray(pinfo[:, :npr], dtype=np.float64).tofile(f)


def _poison(wb):
    """unused slots of every table hold values that fault or mislead whoever reads them"""
    for i in range(wb.B):
        nv, nr, npr, _ = (int(x) for x in wb.counts[i])
        wb.poses[i, nv:] = np.nan
        wb.r_idx[i, nr:] = (I32_MAX, I32_MIN)
        wb.r_val[i, nr:] = np.nan
        wb.p_idx[i, npr:] = I32_MIN
        wb.p_val[i, npr:] = np.nan
    return wb


def test_host_check(driver, tmp_path):
    import localization_amd as la
    batches = []   # (batch, drop, pinfo, expected line)
    wb, drop = F.case_batch(la, "ragged")
    batches.append((_poison(wb), drop, None, "0 0 1 -1"))
    wb, drop = F.case_batch(la, "doubled")                      # a neighbour through a doubled edge is one neighbour
    batches.append((_poison(wb), drop, None, "0 0 1 -1"))
    wb, drop = F.case_batch(la, "last")
    batches.append((_poison(wb), drop, None, "0 0 1 -1"))
    for bad_window, bad_drop in ((0, -1), (7, 3), (3, 2), (5, I32_MAX), (1, I32_MIN)):   # "ragged": nv = 10 4 7 2 9 1 6 3
        wb, drop = F.case_batch(la, "ragged")
        drop = drop.copy(); drop[bad_window] = bad_drop
        batches.append((_poison(wb), drop, None, "0 1 1 -1"))
    wb, drop = F.case_batch(la, "chain10")                      # an inner pose has two neighbours
    drop = drop.copy(); drop[6] = 4
    batches.append((_poison(wb), drop, None, "0 2 1 -1"))
    wb, drop = F.case_batch(la, "chain10")                      # ... and an out-of-range slot elsewhere wins
    drop = drop.copy(); drop[1] = 4; drop[6] = 10
    batches.append((_poison(wb), drop, None, "0 1 1 -1"))
    wb, drop = F.case_batch(la, "missing")                      # pose 1 without its link to pose 0: one neighbour
    batches.append((_poison(wb), np.full(8, 1, dtype=np.int32) * (np.arange(8) % 2 == 0), None, "0 0 1 -1"))
    wb, drop = F.case_batch(la, "fullprior")                    # a full-matrix table: p_val's diagonal is not read
    wb.p_val[:, :, 12:] = 7.0
    batches.append((wb, drop, wb.p_info, "0 0 1 1"))
    wb, drop = F.case_batch(la, "fullprior")
    pinfo = wb.p_info.copy(); pinfo[7, 0, 3 * 6 + 1] = pinfo[7, 0, 1 * 6 + 3] = 1e-300   # a translation-rotation coupling
    batches.append((wb, drop, pinfo, "0 0 1 0"))
    wb, drop = F.case_batch(la, "zprior")
    wb.p_val[4, 0, 16] = 1e-300                                 # rotation information on a diagonal prior
    batches.append((wb, drop, None, "0 0 0 -1"))
    wb, drop = F.case_batch(la, "chain3")
    wb.r_idx[2, 0, 0] = 3                                       # what check_instances refuses never reaches the drop check
    batches.append((wb, drop, None, "2 -1 -1 -1"))
    src = tmp_path / "in.bin"
    with open(src, "wb") as f:
        for wb, drop, pinfo, _ in batches:
            _write(f, wb, drop, len(F.ANCH), pinfo)
    r = subprocess.run([driver, str(src)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-4000:])
    assert r.stdout.splitlines() == [b[3] for b in batches], r.stdout
