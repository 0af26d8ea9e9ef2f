"""CPU checks of the marginal-covariance feature (loc_window_covariance_*): the C ABI declares and exports the entry points and a C
program links against them, and the numpy reference (tests/_covariance_ref.py) reproduces answers known in closed form."""
import ctypes as C
import os
import subprocess

import numpy as np

import localization_amd as la
from localization_amd import _lib

from _covariance_ref import cauchy_rho1, reference_covariance, ros_jacobian

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["loc_window_covariance_host", "loc_window_covariance_resident", "loc_window_last_covariance_ms"]


def test_header_declares_and_library_exports_the_covariance_entry_points(built):
    src = open(os.path.join(ROOT, "include", "localization_amd.h")).read()
    L = la.lib()
    for n in NEW:
        assert f"int {n}(" in src
        assert hasattr(L, n) and n in _lib.EXPORTED_SYMBOLS


def test_c_program_calls_the_covariance_entry_points(tmp_path, built):
    """Strict C99 against the header; without a handle every entry point refuses with LOC_ERR_INVALID (no device needed)."""
    src = tmp_path / "cov_c.c"
    src.write_text('#include "localization_amd.h"\n'
                   "int main(void) {\n"
                   "  int32_t counts[4] = {1, 0, 0, 0}, mask[1], status[1];\n"
                   "  double poses[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0}, cov[36], ms = -1.0;\n"
                   "  if (loc_window_covariance_host(NULL, 1, counts, poses, NULL, NULL, NULL, NULL, NULL, NULL, cov, mask, status) != LOC_ERR_INVALID) return 1;\n"
                   "  if (loc_window_covariance_resident(NULL, NULL, cov, mask, status) != LOC_ERR_INVALID) return 2;\n"
                   "  if (loc_window_last_covariance_ms(NULL, &ms) != LOC_ERR_INVALID) return 3;\n"
                   "  return 0;\n}\n")
    inc = os.path.join(ROOT, "include")
    libdir = os.path.join(ROOT, "localization_amd")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", inc, str(src)])
    exe = tmp_path / "cov_c"
    subprocess.check_call(["gcc", "-std=c99", "-I", inc, str(src), "-o", str(exe), "-L", libdir, "-llocalization_amd", "-Wl,-rpath," + libdir])
    assert subprocess.call([str(exe)]) == 0


def test_reference_single_pose_three_orthogonal_anchors(built):
    """One pose, three anchors on its axes, analytic Jacobians: H_tt = diag(rho'_k info_k), the rotation unconstrained (no lever arm)."""
    from oracle import oracle as O
    anchors = np.array([[2.0, 0, 0], [0, 3.0, 0], [0, 0, 4.0]])
    wb = la.WindowBatch(1, 1, 3, 0, 0)
    wb.add_pose(0, np.zeros(3))
    infos = [100.0, 50.0, 400.0]
    meas = [2.3, 2.9, 4.05]   # residuals 0.3, -0.1, 0.05: rho' != 1
    for k in range(3):
        wb.add_range(0, 0, k, meas[k], infos[k], anchor=True)
    cov, mask = reference_covariance(wb, 0, anchors, O.JAC_ANALYTIC)
    rho = [cauchy_rho1((meas[k] - np.linalg.norm(anchors[k])) ** 2 * infos[k]) for k in range(3)]
    assert all(r < 0.99 for r in rho)
    want = np.zeros((6, 6))
    want[:3, :3] = np.diag([1.0 / (rho[k] * infos[k]) for k in range(3)])
    assert mask[0] == 0x38
    assert np.allclose(cov[0], want, rtol=1e-12, atol=0)


def test_reference_two_pose_chain_against_the_2x2_block_inverse(built):
    """Two poses on the x axis, each ranged to three anchors on its own axes, joined by a range along x (exact measurements: rho' = 1).
    In x, H = [[a + b, -b], [-b, c + b]]: Sigma_0 = (c + b) / ((a + b)(c + b) - b^2), Sigma_1 = (a + b) / (...); y and z decouple."""
    from oracle import oracle as O
    p0, p1 = np.zeros(3), np.array([1.0, 0, 0])
    anchors = np.array([[-3.0, 0, 0], [0, 3.0, 0], [0, 0, 3.0], [4.0, 0, 0], [1.0, -2.0, 0], [1.0, 0, -5.0]])
    wb = la.WindowBatch(1, 2, 7, 0, 0)
    wb.add_pose(0, p0); wb.add_pose(0, p1)
    info0, info1, b = [10.0, 20.0, 30.0], [40.0, 50.0, 60.0], 25.0
    for k in range(3):
        wb.add_range(0, 0, k, np.linalg.norm(p0 - anchors[k]), info0[k], anchor=True)
        wb.add_range(0, 1, 3 + k, np.linalg.norm(p1 - anchors[3 + k]), info1[k], anchor=True)
    wb.add_range(0, 0, 1, 1.0, b)
    cov, mask = reference_covariance(wb, 0, anchors, O.JAC_ANALYTIC)
    a, c = info0[0], info1[0]
    det = (a + b) * (c + b) - b * b
    assert np.allclose(cov[0, :3, :3], np.diag([(c + b) / det, 1 / info0[1], 1 / info0[2]]), rtol=1e-12, atol=1e-15)
    assert np.allclose(cov[1, :3, :3], np.diag([(a + b) / det, 1 / info1[1], 1 / info1[2]]), rtol=1e-12, atol=1e-15)
    assert list(mask) == [0x38, 0x38] and not cov[:, 3:, :].any() and not cov[:, :, 3:].any()
    # the numeric (g2o central-difference) Jacobians agree with the analytic ones to their 1e-7 noise
    cov_n, mask_n = reference_covariance(wb, 0, anchors, O.JAC_NUMERIC_G2O)
    assert list(mask_n) == [0x38, 0x38] and np.allclose(cov_n, cov, rtol=1e-5, atol=0)


def test_ros_frame_map_is_the_derivative_of_the_g2o_increment(built):
    """A = blockdiag(R, 2R) against finite differences of x * fromVectorMQT(d) mapped to world-frame position and rotation angles."""
    from oracle import oracle as O
    from scipy.spatial.transform import Rotation
    L = O.lib()
    rng = np.random.default_rng(3)
    R = Rotation.from_rotvec(rng.normal(0, 1.0, 3)).as_matrix()
    t = rng.normal(0, 1.0, 3)
    A = ros_jacobian(R)
    h = 1e-6
    Afd = np.zeros((6, 6))
    for k in range(6):
        cols = []
        for s in (h, -h):
            d = np.zeros(6); d[k] = s
            Ri, ti = np.zeros(9), np.zeros(3)
            L.og_from_vector_mqt(d.ctypes.data_as(C.POINTER(C.c_double)), Ri.ctypes.data_as(C.POINTER(C.c_double)),
                                 ti.ctypes.data_as(C.POINTER(C.c_double)))
            R2 = R @ Ri.reshape(3, 3)
            t2 = R @ ti + t
            cols.append(np.concatenate([t2, Rotation.from_matrix(R2 @ R.T).as_rotvec()]))
        Afd[:, k] = (cols[0] - cols[1]) / (2 * h)
    assert np.abs(Afd - A).max() < 1e-8
