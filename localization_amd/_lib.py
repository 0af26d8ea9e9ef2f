"""ctypes binding of include/localization_amd.h. Fails loudly when the HIP library is missing."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# (LOCALIZATION_AMD_LIB: an alternative build of the same library, for experiments such as the diagnostic timing build)
_SO = os.environ.get("LOCALIZATION_AMD_LIB") or os.path.join(_HERE, "liblocalization_amd.so")
_LIB = None

LOC_OK = 0
LOC_ERR_NO_DEVICE = -2
JAC_ANALYTIC = 0
JAC_NUMERIC_G2O = 1


class LocalizationAmdError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"localization_amd error {code}: {msg}")
        self.code = code


class SnapshotParams(C.Structure):
    _fields_ = [("maximum_iteration", C.c_int32), ("distance_outlier", C.c_double), ("gate_warmup_epochs", C.c_int32), ("jacobian", C.c_int32),
                ("lanes_per_instance", C.c_int32), ("block_threads", C.c_int32)]


class FusionParams(C.Structure):
    _fields_ = [("maximum_iteration", C.c_int32), ("distance_outlier", C.c_double), ("gate_warmup_epochs", C.c_int32),
                ("antenna_offset", C.c_double * 3), ("block_threads", C.c_int32), ("jacobian", C.c_int32)]


def library_path():
    return _SO


# every symbol include/localization_amd.h declares (tests check the .so exports all of them)
EXPORTED_SYMBOLS = [
    "loc_last_error", "loc_abi_version", "loc_device_count", "loc_shard_bounds", "loc_shard_plan",
    "loc_snapshot_default_params", "loc_snapshot_create", "loc_snapshot_destroy", "loc_snapshot_batch",
    "loc_snapshot_anchor_groups", "loc_snapshot_lanes_per_instance", "loc_snapshot_range_floats",
    "loc_snapshot_set_positions", "loc_snapshot_get_positions", "loc_snapshot_positions_device",
    "loc_snapshot_epochs_done", "loc_snapshot_set_epochs_done",
    "loc_snapshot_pack_ranges_host", "loc_snapshot_solve_device", "loc_snapshot_solve_host",
    "loc_snapshot_solve_host_kmb", "loc_snapshot_solve_device_cov", "loc_snapshot_solve_host_kmb_cov", "loc_host_alloc", "loc_host_free",
    "loc_snapshot_timing_begin", "loc_snapshot_timing_end",
    "loc_window_create", "loc_window_destroy", "loc_window_set_anchors", "loc_window_lds_bytes", "loc_window_solve_host",
    "loc_window_last_kernel_ms", "loc_window_set_endpoint1_offsets", "loc_window_set_prior_information", "loc_window_set_jacobian", "loc_window_set_ordering", "loc_window_set_chain_threshold", "loc_window_last_kernel_kind", "loc_window_set_option", "loc_window_last_host_timing", "loc_window_forest_groups", "loc_window_upload", "loc_window_upload_dev",
    "loc_window_solve_resident", "loc_window_download", "loc_window_poses_device", "loc_window_result_device",
    "loc_window_timing_begin", "loc_window_timing_end",
    "loc_window_covariance_host", "loc_window_covariance_resident", "loc_window_last_covariance_ms", "loc_window_last_covariance_kind", "loc_window_covariance_plan",
    "loc_window_marginal_prior_host", "loc_window_joint_covariance_host", "loc_window_joint_covariance_resident", "loc_window_joint_covariance_plan",
    "loc_window_slide_resident", "loc_window_slide_resident_dev", "loc_window_slide_plain_resident_dev", "loc_window_download_tables",
    "loc_window_edge_chi2_host", "loc_window_edge_chi2_resident", "loc_window_prune_resident",
    "loc_window_publish_resident", "loc_window_path_resident",
    "loc_window_set_message_config", "loc_window_message_rows_dev", "loc_window_push_messages_resident_dev",
    "loc_node_default_config", "loc_node_create", "loc_node_destroy", "loc_node_add_range", "loc_node_add_imu",
    "loc_node_add_pose", "loc_node_add_twist", "loc_node_add_lidar", "loc_node_add_rl_range", "loc_node_solve", "loc_node_get_path",
    "loc_node_number_measurements", "loc_node_last_timing", "loc_node_last_kernel_kind", "loc_node_flush_tail", "loc_node_set_deferred", "loc_node_solve_pending", "loc_nodes_solve_batch",
    "loc_nodes_release_batch_cache",
    "loc_fusion_default_params", "loc_fusion_create", "loc_fusion_destroy", "loc_fusion_set_poses", "loc_fusion_get_poses",
    "loc_fusion_solve_device", "loc_fusion_solve_host", "loc_fusion_solve_host_kmb", "loc_fusion_last_kernel_ms", "loc_fusion_timing_begin", "loc_fusion_timing_end",
    "loc_fusion_solve_device_cov", "loc_fusion_solve_host_kmb_cov",
]


def lib():
    """Load liblocalization_amd.so (built by __graft_entry__.build() / make -C localization_amd/csrc)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(_SO):
        raise LocalizationAmdError(-100, f"{_SO} is missing: build it with `python -c 'import __graft_entry__ as g; "
                                   "g.build()'` (hipcc --offload-arch=gfx950). There is no CPU fallback.")
    L = C.CDLL(_SO)
    vp, dp, fp = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_float)
    L.loc_last_error.restype = C.c_char_p
    L.loc_abi_version.restype = C.c_int32
    L.loc_device_count.restype = C.c_int32
    L.loc_shard_bounds.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.loc_shard_plan.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.c_void_p]
    L.loc_snapshot_default_params.argtypes = [C.POINTER(SnapshotParams)]
    L.loc_snapshot_default_params.restype = None
    L.loc_snapshot_create.argtypes = [C.POINTER(vp), C.c_int32, C.c_int64, C.c_int32, dp, C.POINTER(SnapshotParams)]
    L.loc_snapshot_destroy.argtypes = [vp]
    L.loc_snapshot_batch.argtypes = [vp]; L.loc_snapshot_batch.restype = C.c_int64
    L.loc_snapshot_anchor_groups.argtypes = [vp]; L.loc_snapshot_anchor_groups.restype = C.c_int32
    L.loc_snapshot_lanes_per_instance.argtypes = [vp]; L.loc_snapshot_lanes_per_instance.restype = C.c_int32
    L.loc_snapshot_range_floats.argtypes = [vp, C.c_int32]; L.loc_snapshot_range_floats.restype = C.c_size_t
    L.loc_snapshot_set_positions.argtypes = [vp, dp]
    L.loc_snapshot_get_positions.argtypes = [vp, dp]
    L.loc_snapshot_positions_device.argtypes = [vp]; L.loc_snapshot_positions_device.restype = vp
    L.loc_snapshot_epochs_done.argtypes = [vp]; L.loc_snapshot_epochs_done.restype = C.c_int64
    L.loc_snapshot_set_epochs_done.argtypes = [vp, C.c_int64]
    L.loc_snapshot_pack_ranges_host.argtypes = [vp, C.c_int32, fp, fp, C.c_float]
    L.loc_snapshot_solve_device.argtypes = [vp, C.c_int32, vp, vp, vp, vp, vp, vp]
    L.loc_snapshot_solve_host.argtypes = [vp, C.c_int32, fp, fp, dp, dp, C.POINTER(C.c_uint8)]
    L.loc_snapshot_solve_host_kmb.argtypes = [vp, C.c_int32, vp, vp, vp, vp, vp]
    L.loc_snapshot_solve_device_cov.argtypes = [vp, C.c_int32] + [vp] * 9
    L.loc_snapshot_solve_host_kmb_cov.argtypes = [vp, C.c_int32] + [vp] * 8
    L.loc_host_alloc.argtypes = [C.POINTER(vp), C.c_size_t]
    L.loc_host_free.argtypes = [vp]
    L.loc_snapshot_timing_begin.argtypes = [vp, C.c_int32]
    L.loc_snapshot_timing_end.argtypes = [vp, C.POINTER(C.c_int32), dp, dp]
    ip = C.POINTER(C.c_int32)
    L.loc_window_create.argtypes = [C.POINTER(vp), C.c_int32, C.c_int64, vp, C.c_int32, dp, C.c_int32]
    L.loc_window_destroy.argtypes = [vp]
    L.loc_window_set_anchors.argtypes = [vp, C.c_int32, dp]
    L.loc_window_lds_bytes.argtypes = [vp]; L.loc_window_lds_bytes.restype = C.c_size_t
    L.loc_window_solve_host.argtypes = [vp, C.c_int64, ip, dp, ip, dp, ip, dp, ip, dp, dp]
    L.loc_window_last_kernel_ms.argtypes = [vp, dp]
    L.loc_window_set_jacobian.argtypes = [vp, C.c_int32]
    L.loc_window_set_endpoint1_offsets.argtypes = [vp, C.c_int64, dp]
    L.loc_window_set_prior_information.argtypes = [vp, C.c_int64, dp]
    L.loc_window_set_ordering.argtypes = [vp, C.c_int32]
    L.loc_window_set_chain_threshold.argtypes = [vp, C.c_int64]
    L.loc_window_last_kernel_kind.argtypes = [vp, ip]
    L.loc_window_last_host_timing.argtypes = [vp, dp]
    L.loc_window_last_covariance_kind.argtypes = [vp, ip]
    L.loc_window_forest_groups.argtypes =[vp, ip, C.POINTER(C.c_int64)]
    L.loc_window_upload.argtypes = [vp, C.c_int64, ip, dp, ip, dp, ip, dp, ip, dp]
    L.loc_window_upload_dev.argtypes = [vp, vp, C.c_int64] + [vp] * 9
    L.loc_window_solve_resident.argtypes = [vp, vp]
    L.loc_window_download.argtypes = [vp, dp, dp]
    L.loc_window_poses_device.argtypes = [vp]; L.loc_window_poses_device.restype = vp
    L.loc_window_result_device.argtypes = [vp]; L.loc_window_result_device.restype = vp
    L.loc_window_timing_begin.argtypes = [vp, C.c_int32]
    L.loc_window_timing_end.argtypes = [vp, ip, dp, dp]
    L.loc_window_covariance_host.argtypes = [vp, C.c_int64, ip, dp, ip, dp, ip, dp, ip, dp, dp, ip, ip]
    L.loc_window_marginal_prior_host.argtypes = [vp, C.c_int64, ip, dp, ip, dp, ip, dp, ip, dp, ip, ip, dp, dp, dp, ip, ip]
    L.loc_window_covariance_resident.argtypes = [vp, vp, vp, vp, vp]
    L.loc_window_last_covariance_ms.argtypes = [vp, dp]
    L.loc_window_covariance_plan.argtypes = [vp, C.c_int64, ip, ip, ip, C.POINTER(C.c_int64), C.POINTER(C.c_size_t)]
    L.loc_window_joint_covariance_host.argtypes = [vp, C.c_int64, ip, dp, ip, dp, ip, dp, ip, dp, C.c_int32, ip, ip, dp, ip, ip, dp]
    L.loc_window_joint_covariance_resident.argtypes = [vp, vp, C.c_int32, ip, ip, vp, vp, vp, vp]
    L.loc_window_joint_covariance_plan.argtypes = [vp, C.c_int64, ip, ip, ip, C.c_int32, ip, ip, C.POINTER(C.c_int64), C.POINTER(C.c_size_t)]
    L.loc_window_set_option.argtypes = [vp, C.c_char_p, C.c_int64]
    L.loc_window_slide_resident.argtypes = [vp, vp, ip, dp, C.c_int32, ip, ip, dp, C.c_int32, ip, dp, vp, vp, vp, vp]
    L.loc_window_slide_resident_dev.argtypes = [vp, vp, vp, vp, C.c_int32, vp, vp, vp, C.c_int32, vp, vp, vp, vp, vp, vp, vp]
    L.loc_window_slide_plain_resident_dev.argtypes = [vp, vp, vp, vp, C.c_int32, vp, vp, vp, C.c_int32, vp, vp, C.c_int32, vp, vp, vp, vp, vp]
    L.loc_window_download_tables.argtypes = [vp, ip, dp, ip, dp, ip, dp, ip, dp, dp]
    L.loc_window_edge_chi2_host.argtypes = [vp, C.c_int64, ip, dp, ip, dp, ip, dp, ip, dp, dp, dp, dp, dp, ip]
    L.loc_window_edge_chi2_resident.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.loc_window_prune_resident.argtypes = [vp, vp, C.c_double, C.c_int32, vp, vp]
    L.loc_window_publish_resident.argtypes = [vp, vp, C.c_double, C.c_int32, vp, vp, vp, vp, vp]
    L.loc_window_path_resident.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int32, vp, vp]
    L.loc_window_set_message_config.argtypes =[vp, vp, C.c_int32, dp]
    L.loc_window_message_rows_dev.argtypes = [vp, vp, C.c_int32, vp, vp]
    L.loc_window_push_messages_resident_dev.argtypes = [vp, vp, C.c_int32, vp, vp, vp, vp]
    L.loc_fusion_default_params.argtypes = [C.POINTER(FusionParams)]; L.loc_fusion_default_params.restype = None
    L.loc_fusion_create.argtypes = [C.POINTER(vp), C.c_int32, C.c_int64, C.c_int32, dp, C.POINTER(FusionParams)]
    L.loc_fusion_destroy.argtypes = [vp]
    L.loc_fusion_set_poses.argtypes = [vp, dp]
    L.loc_fusion_get_poses.argtypes = [vp, dp]
    L.loc_fusion_solve_device.argtypes = [vp, C.c_int32] + [vp] * 7
    L.loc_fusion_solve_device_cov.argtypes = [vp, C.c_int32] + [vp] * 10
    L.loc_fusion_solve_host.argtypes = [vp, C.c_int32, fp, fp, dp, dp, dp, C.POINTER(C.c_uint8)]
    L.loc_fusion_solve_host_kmb.argtypes = [vp, C.c_int32] + [vp] * 6
    L.loc_fusion_solve_host_kmb_cov.argtypes = [vp, C.c_int32] + [vp] * 9
    L.loc_fusion_last_kernel_ms.argtypes = [vp, dp]
    L.loc_fusion_timing_begin.argtypes = [vp, C.c_int32]
    L.loc_fusion_timing_end.argtypes = [vp, ip, dp, dp]
    _LIB = L
    return L


def unpack_covariance(packed, n):
    """[K][n(n+1)/2][B] row-major upper triangles (the covariance outputs' layout) -> full symmetric [K][B][n][n]"""
    import numpy as np
    p = np.asarray(packed)
    K, T, B = p.shape
    assert T == n * (n + 1) // 2
    out = np.empty((K, B, n, n), dtype=p.dtype)
    i = 0
    for r in range(n):
        for c in range(r, n):
            out[:, :, r, c] = p[:, i, :]
            out[:, :, c, r] = p[:, i, :]
            i += 1
    return out


def check(rc):
    if rc != LOC_OK:
        raise LocalizationAmdError(rc, lib().loc_last_error().decode(errors="replace"))


def abi_version():
    return lib().loc_abi_version()


def device_count():
    return lib().loc_device_count()


class Handle:
    """What the three solver classes share: the lifetime of a loc_<kind>_* handle (self.h, self.L; _prefix names the kind) and the
    HIP-event timing of its launches."""
    _prefix = None   # "loc_snapshot" / "loc_fusion" / "loc_window"

    def _fn(self, name):
        return getattr(self.L, f"{self._prefix}_{name}")

    def close(self):
        if getattr(self, "h", None):
            self._fn("destroy")(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- HIP-event kernel timing -------------------------------------------------------------------
    def timing_begin(self, max_launches):
        check(self._fn("timing_begin")(self.h, int(max_launches)))

    def timing_end(self):
        n = C.c_int32(); tot = C.c_double(); avg = C.c_double()
        check(self._fn("timing_end")(self.h, C.byref(n), C.byref(tot), C.byref(avg)))
        return n.value, tot.value, avg.value


class EpochSolver(Handle):
    """The snapshot and fusion solvers (self.B tags on GPU self.device): page-locked host arrays that live as long as the handle,
    and the per-update outputs — the state is [K][n_state][B], a covariance [K][n_cov][B]."""

    def close(self):
        if getattr(self, "h", None):
            for p in getattr(self, "_pinned", []):
                self.L.loc_host_free(p)
            self._pinned = []
        super().close()

    def pinned(self, shape, dtype):
        """A page-locked numpy array (loc_host_alloc); freed when the solver is closed."""
        import numpy as np
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        check(self.L.loc_host_alloc(C.byref(p), n))
        self._pinned = getattr(self, "_pinned", []) + [p]
        return np.frombuffer((C.c_char * n).from_address(p.value), dtype=dtype).reshape(shape)

    def _device_outputs(self, K, n_state, n_cov, trials, covariance):
        """(state, chi2, trials) device tensors; with covariance also (cov f64, mask [K][B] i32, status [K][B] i32)"""
        import torch as t
        dev = t.device("cuda", self.device)
        out = (t.empty((K, n_state, self.B), dtype=t.float64, device=dev), t.empty((K, self.B), dtype=t.float64, device=dev),
               t.empty((K, self.B), dtype=t.uint8, device=dev) if trials else None)
        if covariance:
            out += (t.empty((K, n_cov, self.B), dtype=t.float64, device=dev),) + tuple(t.empty((K, self.B), dtype=t.int32, device=dev) for _ in range(2))
        return out

    def _host_outputs(self, K, n_state, n_cov, covariance):
        import numpy as np
        out = (np.empty((K, n_state, self.B)), np.empty((K, self.B)), np.empty((K, self.B), dtype=np.uint8))
        if covariance:
            out += (np.empty((K, n_cov, self.B)), np.empty((K, self.B), dtype=np.int32), np.empty((K, self.B), dtype=np.int32))
        return out

    def _cov_device_args(self, outs, K, n_cov, dev):
        """all three covariance output tensors or none: their device pointers, [] if none"""
        import torch as t
        given = [x is not None for x in outs]
        if not any(given):
            return []
        if not all(given):
            raise ValueError("out_cov, out_cov_mask and out_cov_status go together: pass all three or none")
        cov, mask, status = outs
        assert tuple(cov.shape) == (K, n_cov, self.B) and cov.dtype == t.float64 and cov.is_contiguous() and cov.device == dev
        for x in (mask, status):
            assert tuple(x.shape) == (K, self.B) and x.dtype == t.int32 and x.is_contiguous() and x.device == dev
        return [cov.data_ptr(), mask.data_ptr(), status.data_ptr()]

    def _cov_host_args(self, outs, K, n_cov):
        import numpy as np
        cov, mask, status = outs
        assert cov.shape == (K, n_cov, self.B) and cov.dtype == np.float64 and cov.flags.c_contiguous
        for x in (mask, status):
            assert x.shape == (K, self.B) and x.dtype == np.int32 and x.flags.c_contiguous
        return [cov.ctypes.data, mask.ctypes.data, status.ctypes.data]
