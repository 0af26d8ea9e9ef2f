"""CPU checks of the per-update covariances of the snapshot and fusion solvers (loc_snapshot_solve_*_cov, loc_fusion_solve_*_cov): the C ABI
declares and exports the entry points, a strict C99 program calls them, and the numpy reference (tests/_snapshot_covariance_ref.py)
reproduces answers known in closed form."""
import os
import subprocess

import numpy as np

import localization_amd as la
from localization_amd import _lib

from _covariance_ref import cauchy_rho1
from _snapshot_covariance_ref import fusion_reference, snapshot_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["loc_snapshot_solve_device_cov", "loc_snapshot_solve_host_kmb_cov", "loc_fusion_solve_device_cov", "loc_fusion_solve_host_kmb_cov"]


def test_header_declares_and_library_exports_the_update_covariance_entry_points(built):
    src = open(os.path.join(ROOT, "include", "localization_amd.h")).read()
    L = la.lib()
    for n in NEW:
        assert f"int {n}(" in src
        assert hasattr(L, n) and n in _lib.EXPORTED_SYMBOLS
    assert la.abi_version() == 4


def test_c_program_calls_the_update_covariance_entry_points(tmp_path, built):
    """Strict C99 against the header; without a handle every entry point refuses with LOC_ERR_INVALID (no device needed)."""
    src = tmp_path / "scov_c.c"
    src.write_text('#include "localization_amd.h"\n'
                   "int main(void) {\n"
                   "  float d[16] = {0}, e[16] = {0};\n"
                   "  double imu[8] = {0}, pos[21], chi2[1], cov[21];\n"
                   "  uint8_t tr[1];\n"
                   "  int32_t mask[1], status[1];\n"
                   "  if (loc_snapshot_solve_device_cov(NULL, 1, d, e, pos, chi2, tr, cov, mask, status, NULL) != LOC_ERR_INVALID) return 1;\n"
                   "  if (loc_snapshot_solve_host_kmb_cov(NULL, 1, d, e, pos, chi2, tr, cov, mask, status) != LOC_ERR_INVALID) return 2;\n"
                   "  if (loc_fusion_solve_device_cov(NULL, 1, d, e, imu, pos, chi2, tr, cov, mask, status, NULL) != LOC_ERR_INVALID) return 3;\n"
                   "  if (loc_fusion_solve_host_kmb_cov(NULL, 1, d, e, imu, pos, chi2, tr, cov, mask, status) != LOC_ERR_INVALID) return 4;\n"
                   "  return 0;\n}\n")
    inc = os.path.join(ROOT, "include")
    libdir = os.path.join(ROOT, "localization_amd")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", inc, str(src)])
    exe = tmp_path / "scov_c"
    subprocess.check_call(["gcc", "-std=c99", "-I", inc, str(src), "-o", str(exe), "-L", libdir, "-llocalization_amd", "-Wl,-rpath," + libdir])
    assert subprocess.call([str(exe)]) == 0


def _one(dist, err, pos, anchors, mode, gate=0.0):
    """the reference for one tag and one epoch at `pos`, the prior = pos"""
    d = np.asarray(dist, np.float32).reshape(1, -1, 1)
    e = np.asarray(err, np.float32).reshape(1, -1, 1)
    p = np.asarray(pos, float).reshape(3, 1)
    cov, mask, ok, nact = snapshot_reference(anchors, d, e, p, p.reshape(1, 3, 1), mode, gate=gate, gate_from_epoch=0)
    return cov[0, 0], int(mask[0, 0]), bool(ok[0, 0]), int(nact[0, 0])


def test_reference_three_orthogonal_anchors_is_the_inverse_weighted_information(built):
    """A tag at the origin, three anchors on its axes, no gate: H = diag(rho'_m Omega_m), so Sigma = diag(1 / (rho'_m Omega_m)); both
    Jacobian modes."""
    from oracle import oracle as O
    anchors = np.array([[2.0, 0, 0], [0, 3.0, 0], [0, 0, 4.0]])
    dist = np.array([2.25, 2.875, 4.0625], np.float32)   # residuals 0.25, -0.125, 0.0625 (exact in float32): rho' != 1
    err = np.array([0.125, 0.25, 0.0625], np.float32)
    infos = 1.0 / err.astype(float) ** 2
    rho = [cauchy_rho1((float(dist[m]) - np.linalg.norm(anchors[m])) ** 2 * infos[m]) for m in range(3)]
    assert all(r < 0.9 for r in rho)
    want = np.diag([1.0 / (rho[m] * infos[m]) for m in range(3)])
    cov, mask, ok, nact = _one(dist, err, np.zeros(3), anchors, O.JAC_ANALYTIC)
    assert ok and mask == 0 and nact == 3
    assert np.allclose(cov, want, rtol=1e-12, atol=0)
    cov_n, mask_n, ok_n, _ = _one(dist, err, np.zeros(3), anchors, O.JAC_NUMERIC_G2O)
    assert ok_n and mask_n == 0 and np.allclose(cov_n, want, rtol=1e-6, atol=0)


def test_reference_tag_in_the_anchors_plane_masks_that_coordinate(built):
    """Four anchors and the tag in the plane z = 1: every range's dz is exactly 0, so the z column of every Jacobian (analytic, and the
    central difference: (+d)^2 == (-d)^2) is exactly 0 — z is excluded (bit 2), its entries 0; x, y regular."""
    from oracle import oracle as O
    anchors = np.array([[3.0, -3.0, 1.0], [3.0, 3.0, 1.0], [-3.0, 3.0, 1.0], [-3.0, -3.0, 1.0]])
    pos = np.array([0.5, -0.25, 1.0])
    dist = np.linalg.norm(anchors - pos, axis=1) + np.array([0.02, -0.01, 0.03, 0.0])
    for mode in (O.JAC_ANALYTIC, O.JAC_NUMERIC_G2O):
        cov, mask, ok, nact = _one(dist, np.full(4, 0.055), pos, anchors, mode)
        assert ok and mask == 0b100 and nact == 4
        assert not cov[2].any() and not cov[:, 2].any()
        assert np.all(np.linalg.eigvalsh(cov[:2, :2]) > 0)


def test_reference_two_anchors_are_singular(built):
    """Two ranges constrain two directions of a 3-D position: the LDL^T's last pivot is rounding noise and fails the relative test."""
    from oracle import oracle as O
    anchors = np.array([[3.0, -3.0, 0.0], [3.0, 3.0, 2.0]])
    pos = np.array([0.5, -0.25, 1.2])
    dist = np.linalg.norm(anchors - pos, axis=1) + 0.01
    for mode in (O.JAC_ANALYTIC, O.JAC_NUMERIC_G2O):
        cov, mask, ok, nact = _one(dist, np.full(2, 0.055), pos, anchors, mode)
        assert not ok and mask == 0 and nact == 2 and np.isnan(cov).all()


def test_reference_no_active_range_masks_everything(built):
    """Every range gated away: an all-zero diagonal, every bit set, zeros, not singular (the same rule as a fully masked window pose)."""
    from oracle import oracle as O
    anchors = np.array([[3.0, -3.0, 0.0], [3.0, 3.0, 2.0], [-3.0, 3.0, 0.0], [-3.0, -3.0, 2.0]])
    pos = np.array([0.5, -0.25, 1.2])
    dist = np.linalg.norm(anchors - pos, axis=1) + 5.0
    cov, mask, ok, nact = _one(dist, np.full(4, 0.055), pos, anchors, O.JAC_ANALYTIC, gate=1.0)
    assert ok and mask == 0b111 and nact == 0 and not cov.any()


def test_fusion_reference_zero_lever_arm_decouples_rotation_from_the_ranges(built):
    """Without a lever arm the ranges do not see the rotation: H is block diagonal, the rotation block is the IMU prior's
    diag(1/c) through the analytic prior Jacobian (the identity at an error-free prior), the translation block the snapshot one."""
    from oracle import oracle as O
    anchors = np.array([[3.0, -3.0, 0.0], [3.0, 3.0, 2.0], [-3.0, 3.0, 0.0], [-3.0, -3.0, 2.0]])
    t = np.array([0.5, -0.25, 1.2])
    c = np.array([4e-6, 5e-6, 6e-6])
    imu = np.zeros((1, 1, 8)); imu[0, 0, 3] = 1.0; imu[0, 0, 4:7] = c
    dist = (np.linalg.norm(anchors - t, axis=1) + np.array([0.02, -0.01, 0.03, 0.0])).astype(np.float32).reshape(1, 4, 1)
    err = np.full((1, 4, 1), 0.055, np.float32)
    pose = np.array([*t, 0, 0, 0, 1.0]).reshape(7, 1)
    cov, mask, ok, nact = fusion_reference(anchors, np.zeros(3), dist, err, imu, pose, pose.reshape(1, 7, 1), O.JAC_ANALYTIC, gate_from_epoch=0)
    assert ok[0, 0] and mask[0, 0] == 0 and nact[0, 0] == 4
    S = cov[0, 0]
    assert not S[:3, 3:].any()
    assert np.allclose(np.diag(S[3:, 3:]), c, rtol=1e-12) and not (S[3:, 3:] - np.diag(np.diag(S[3:, 3:]))).any()
    snap, _, _, _ = snapshot_reference(anchors, dist, err, t.reshape(3, 1), t.reshape(1, 3, 1), O.JAC_ANALYTIC, gate_from_epoch=0)
    assert np.allclose(S[:3, :3], snap[0, 0], rtol=1e-12, atol=0)


def test_unpack_covariance_is_the_row_major_upper_triangle():
    rng = np.random.default_rng(0)
    for n in (3, 6):
        full = rng.normal(size=(2, 5, n, n)); full = full + full.transpose(0, 1, 3, 2)
        iu = np.triu_indices(n)
        packed = np.ascontiguousarray(full[:, :, iu[0], iu[1]].transpose(0, 2, 1))   # [K][n(n+1)/2][B]
        assert np.array_equal(_lib.unpack_covariance(packed, n), full)
