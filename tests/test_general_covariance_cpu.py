"""CPU-side checks behind envelope_covariance_kernel.hip (option "covariance_general"): loc_window_covariance_plan — declared, exported,
callable from C without a device, and equal to a numpy count of the envelope —, the envelope-closure identity the kernel rests on (a numpy
model of its block LDL^T and restricted selected inversion against np.linalg.inv), and the regularity of every input of
tests/test_gpu_general_covariance.py by the reference alone."""
import os
import subprocess

import numpy as np
import pytest

import localization_amd as la
from localization_amd.window import covariance_plan
import _general_cov_inputs as G
from _covariance_ref import hessian

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _structure_batch(kind, n):
    """one window of n poses with the named pose-to-pose structure (the plan reads nothing but counts and index tables)"""
    wb = la.WindowBatch(1, n, 2 * n, 0, n)
    wb.counts[0, 0] = n
    if kind in ("chain", "loop"):
        for k in range(1, n):
            wb.add_range(0, k, 0, 1.0, 1.0, anchor=True)           # (a fixed endpoint: no block)
            if k % 2: wb.add_range(0, k - 1, k, 0.0, 1.0)
            else: wb.add_se3(0, k, k - 1, np.zeros(3), np.eye(3), np.eye(6))
        if kind == "loop": wb.add_se3(0, n - 1, 0, np.zeros(3), np.eye(3), np.eye(6))
    elif kind == "leaves_first":
        for k in range(n - 1): wb.add_se3(0, n - 1, k, np.zeros(3), np.eye(3), np.eye(6))
    elif kind == "key_first":
        for k in range(1, n): wb.add_se3(0, 0, k, np.zeros(3), np.eye(3), np.eye(6))
    return wb


@pytest.mark.parametrize("kind,n,closed", [("chain", 9, lambda n: 2 * n - 1), ("leaves_first", 11, lambda n: 2 * n - 1),
                                           ("key_first", 11, lambda n: n * (n + 1) // 2), ("loop", 9, lambda n: 3 * n - 3)])
def test_plan_counts_the_envelope(built, kind, n, closed):
    wb = _structure_batch(kind, n)
    blocks, nbytes = covariance_plan(wb)
    assert blocks == G.envelope_blocks(wb, 0) == closed(n)
    assert nbytes == ((blocks + n) * 36 + n * 6) * 8


def test_plan_takes_the_largest_window_and_refuses_bad_tables(built):
    wb = G.mixed_batch(la)
    blocks, nbytes = covariance_plan(wb)
    per_window = [G.envelope_blocks(wb, i) for i in range(wb.B)]
    assert blocks == max(per_window) == G.MIXED_NV[2] * (G.MIXED_NV[2] + 1) // 2   # the key-first star
    assert per_window[1] == 2 * G.MIXED_NV[1] - 1
    assert nbytes == wb.B * ((blocks + 24) * 36 + 24 * 6) * 8
    bad = wb.copy()
    bad.s_idx[1, 0, 1] = 24
    with pytest.raises(la.LocalizationAmdError) as ex:
        covariance_plan(bad)
    assert ex.value.code == -1


def test_plan_is_callable_from_c_without_a_device(tmp_path, built):
    src = tmp_path / "plan_c.c"
    src.write_text('#include "localization_amd.h"\n'
                   "int main(void) {\n"
                   "  loc_window_caps caps = {5, 4, 0, 1, -1};\n"
                   "  const int32_t counts[4] = {5, 4, 0, 1};\n"
                   "  const int32_t r_idx[8] = {0, 1, 2, 1, 2, 3, 4, -1};   /* 0-1, 1-2, 2-3, pose 4 to an anchor */\n"
                   "  const int32_t s_idx[4] = {4, 1, 1, 0};                /* 4-1: row 4 reaches back to slot 1 */\n"
                   "  int64_t blocks = -1; size_t bytes = 0;\n"
                   "  if (loc_window_covariance_plan(&caps, 1, counts, r_idx, s_idx, &blocks, &bytes) != LOC_OK) return 1;\n"
                   "  if (blocks != 1 + 2 + 2 + 2 + 4) return 2;\n"
                   "  if (bytes != ((11 + 5) * 36 + 5 * 6) * sizeof(double)) return 3;\n"
                   "  if (loc_window_covariance_plan(&caps, 1, counts, r_idx, s_idx, 0, &bytes) != LOC_ERR_INVALID) return 4;\n"
                   "  return 0;\n}\n")
    inc = os.path.join(ROOT, "include")
    libdir = os.path.join(ROOT, "localization_amd")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", inc, str(src)])
    exe = tmp_path / "plan_c"
    subprocess.check_call(["gcc", "-std=c99", "-I", inc, str(src), "-o", str(exe), "-L", libdir, "-llocalization_amd", "-Wl,-rpath," + libdir])
    assert subprocess.call([str(exe)]) == 0


@pytest.fixture(scope="module")
def solved(built):
    """every input family at its oracle-solved poses, and its H there: name -> (batch, [H per window])"""
    from oracle import oracle as O
    from _oracle_window import oracle_solve_instance
    out = {}
    for name in G.CASES:
        wb = G.case_batch(la, name)
        Hs = []
        for i in range(wb.B):
            nv = int(wb.counts[i, 0])
            wb.poses[i, :nv] = oracle_solve_instance(wb, i, G.ANCH, jac_mode=O.JAC_NUMERIC_G2O)[0]
            Hs.append(hessian(wb, i, G.ANCH, O.JAC_NUMERIC_G2O))
        out[name] = (wb, Hs)
    return out


@pytest.mark.parametrize("name", list(G.CASES))
def test_inputs_are_regular_by_the_reference(solved, name):
    """At the oracle-solved poses every LDL^T pivot of the reference's H_kept is above 1e-9 of its diagonal entry: two orders clear of the
    kernel's 1e-11 rule."""
    wb, Hs = solved[name]
    for i, H in enumerate(Hs):
        assert G.min_relative_pivot(H) > 1e-9, (name, i)


@pytest.mark.parametrize("name", list(G.CASES))
def test_envelope_model_reproduces_the_inverse(solved, name):
    """The block LDL^T on the envelope of the caller's pose order plus the selected inversion restricted to struct(j) gives the diagonal
    blocks of inv(H_kept) to 1e-10 — without ever reading a block outside the envelope (the model keeps those NaN)."""
    wb, Hs = solved[name]
    for i, H in enumerate(Hs):
        nv = int(wb.counts[i, 0])
        keep = np.diag(H) != 0
        want = np.zeros_like(H)
        want[np.ix_(keep, keep)] = np.linalg.inv(H[np.ix_(keep, keep)])
        Hm = H.copy()
        Hm[~keep, ~keep] = 1.0
        got, pivot = G.envelope_selected_inverse(Hm, G.envelope_first(nv, G.window_pairs(wb, i)))
        assert pivot > 1e-9
        for v in range(nv):
            k6 = keep[6 * v:6 * v + 6]
            g, r = got[v][np.ix_(k6, k6)], want[6 * v:6 * v + 6, 6 * v:6 * v + 6][np.ix_(k6, k6)]
            assert np.linalg.norm(g - r) <= 1e-10 * np.linalg.norm(r), (name, i, v)
