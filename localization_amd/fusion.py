"""Batched fusion snapshot solver (BASELINE config 3): Python harness over loc_fusion_*."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import FusionParams, check, lib   # (FusionParams: part of this module's surface)
from .snapshot import pack_ranges


class FusionSolver(_lib.EpochSolver):
    """B tags, each a 6-DoF pose: M <= 8 anchor ranges with an antenna lever arm + an IMU rotation prior per epoch."""
    _prefix = "loc_fusion"

    def __init__(self, anchors, batch, antenna_offset=(0.0, 0.0, 0.0), maximum_iteration=10, distance_outlier=3.0,
                 gate_warmup_epochs=1, block_threads=0, device=0, jacobian="numeric"):
        L = lib()
        if L.loc_device_count() <= 0:
            raise _lib.LocalizationAmdError(_lib.LOC_ERR_NO_DEVICE, "no HIP device visible: localization_amd has no CPU fallback")
        anchors = np.ascontiguousarray(anchors, dtype=np.float64)
        self.M, self.B, self.device, self.L = anchors.shape[0], int(batch), int(device), L
        prm = FusionParams()
        L.loc_fusion_default_params(C.byref(prm))
        prm.maximum_iteration = int(maximum_iteration); prm.distance_outlier = float(distance_outlier)
        prm.gate_warmup_epochs = int(gate_warmup_epochs); prm.block_threads = int(block_threads)
        prm.jacobian = _lib.JAC_NUMERIC_G2O if jacobian in ("numeric", _lib.JAC_NUMERIC_G2O) else _lib.JAC_ANALYTIC
        prm.antenna_offset[0], prm.antenna_offset[1], prm.antenna_offset[2] = [float(v) for v in antenna_offset]
        h = C.c_void_p()
        check(L.loc_fusion_create(C.byref(h), self.device, self.B, self.M, anchors.ctypes.data_as(C.POINTER(C.c_double)), C.byref(prm)))
        self.h = h

    def set_poses(self, pose_7b):
        p = np.ascontiguousarray(pose_7b, dtype=np.float64)
        assert p.shape == (7, self.B)
        check(self.L.loc_fusion_set_poses(self.h, p.ctypes.data_as(C.POINTER(C.c_double))))

    def get_poses(self):
        p = np.zeros((7, self.B))
        check(self.L.loc_fusion_get_poses(self.h, p.ctypes.data_as(C.POINTER(C.c_double))))
        return p

    def solve(self, dist_kmb, err_kmb, imu_kb8):
        """Host path. dist/err [K][M][B] f32, imu [K][B][8] f64. Returns (pose[K,7,B], chi2[K,B], trials[K,B])."""
        d = pack_ranges(dist_kmb, 0.0); e = pack_ranges(err_kmb, 0.0)
        K = d.shape[0]
        assert d.shape == (K, 2, self.B, 4), "the fusion kernel takes up to 8 anchors"
        imu = np.ascontiguousarray(imu_kb8, dtype=np.float64)
        assert imu.shape == (K, self.B, 8)
        pose = np.empty((K, 7, self.B)); chi2 = np.empty((K, self.B)); trials = np.empty((K, self.B), dtype=np.uint8)
        fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
        check(self.L.loc_fusion_solve_host(self.h, K, d.ctypes.data_as(fp), e.ctypes.data_as(fp), imu.ctypes.data_as(dp),
                                           pose.ctypes.data_as(dp), chi2.ctypes.data_as(dp), trials.ctypes.data_as(C.POINTER(C.c_uint8))))
        return pose, chi2, trials

    def solve_stream(self, dist_kmb, err_kmb, imu_kb8, covariance=False, out=None):
        """The pipelined host path (loc_fusion_solve_host_kmb): natural [K][M][B] arrays, tiles packed on the GPU.
        covariance=True (loc_fusion_solve_host_kmb_cov) returns (pose, chi2, trials, cov, mask, status) with cov unpacked to full
        symmetric [K][B][6][6] in [tx ty tz qx qy qz]; `out` = (pose, chi2, trials, cov [K][21][B], mask, status) to reuse (e.g. pinned)
        output arrays there."""
        d = np.ascontiguousarray(dist_kmb, dtype=np.float32); e = np.ascontiguousarray(err_kmb, dtype=np.float32)
        imu = np.ascontiguousarray(imu_kb8, dtype=np.float64)
        K = d.shape[0]
        assert d.shape == (K, self.M, self.B) and e.shape == d.shape and imu.shape == (K, self.B, 8)
        if out is None or not covariance:   # (`out` is for the covariance form)
            out = self._host_outputs(K, 7, 21, covariance)
        pose, chi2, trials = out[:3]
        assert pose.shape == (K, 7, self.B) and pose.dtype == np.float64 and chi2.shape == (K, self.B) and trials.shape == (K, self.B)
        cov = self._cov_host_args(out[3:], K, 21) if covariance else []
        fn = self.L.loc_fusion_solve_host_kmb_cov if covariance else self.L.loc_fusion_solve_host_kmb
        check(fn(self.h, K, d.ctypes.data, e.ctypes.data, imu.ctypes.data, pose.ctypes.data, chi2.ctypes.data, trials.ctypes.data, *cov))
        return (pose, chi2, trials, _lib.unpack_covariance(out[3], 6), out[4], out[5]) if covariance else (pose, chi2, trials)

    def alloc_outputs(self, K, trials=True, covariance=False):
        """(pose [K][7][B], chi2, trials) device tensors; with covariance=True also (cov [K][21][B] f64, mask [K][B] i32, status [K][B] i32)."""
        return self._device_outputs(K, 7, 21, trials, covariance)

    def solve_device(self, dist_tiles, err_tiles, imu, out_pose, out_chi2, out_trials=None, out_cov=None, out_cov_mask=None,
                     out_cov_status=None):
        """Asynchronous on the current torch stream.  out_cov / out_cov_mask / out_cov_status (all three or none): each update's
        marginal covariance of the pose (loc_fusion_solve_device_cov: [K][21][B], [K][B] mask bits, [K][B] status)."""
        import torch
        K = dist_tiles.shape[0]
        assert tuple(dist_tiles.shape) == (K, 2, self.B, 4) and tuple(imu.shape) == (K, self.B, 8)
        assert tuple(out_pose.shape) == (K, 7, self.B) and tuple(out_chi2.shape) == (K, self.B)
        for x in (dist_tiles, err_tiles, imu, out_pose, out_chi2):
            assert x.is_contiguous()
        cov = self._cov_device_args((out_cov, out_cov_mask, out_cov_status), K, 21, dist_tiles.device)
        fn = self.L.loc_fusion_solve_device_cov if cov else self.L.loc_fusion_solve_device
        check(fn(self.h, K, dist_tiles.data_ptr(), err_tiles.data_ptr(), imu.data_ptr(), out_pose.data_ptr(), out_chi2.data_ptr(),
                 out_trials.data_ptr() if out_trials is not None else None, *cov,
                 C.c_void_p(torch.cuda.current_stream(dist_tiles.device).cuda_stream)))

    def last_kernel_ms(self):
        ms = C.c_double()
        check(self.L.loc_fusion_last_kernel_ms(self.h, C.byref(ms)))
        return ms.value
