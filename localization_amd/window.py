"""Batched sliding-window graph solver: Python harness over loc_window_* (include/localization_amd.h)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib


class WindowCaps(C.Structure):
    _fields_ = [("nv_max", C.c_int32), ("nr_max", C.c_int32), ("np_max", C.c_int32), ("ns_max", C.c_int32), ("bw_max", C.c_int32)]


class MessageConfig(C.Structure):
    _fields_ = [("trajectory_length", C.c_int32), ("maximum_velocity", C.c_double), ("distance_outlier", C.c_double)]


_IP, _DP = C.POINTER(C.c_int32), C.POINTER(C.c_double)
_I32, _F64 = np.dtype(np.int32), np.dtype(np.float64)


def _inv_iso(R, t):
    Ri = R.T
    return Ri, -Ri @ t


def _dev(t):
    """device pointer argument from None, an int or an object with data_ptr()"""
    return C.c_void_p(None if t is None else t.data_ptr() if hasattr(t, "data_ptr") else int(t))


def _stream(stream):
    """stream argument from None (the handle's own) or a torch stream"""
    return None if stream is None else C.c_void_p(stream.cuda_stream)


def _new_rows(rows, n):
    """(capacity, *n device pointers) of a new_ranges / new_priors / new_se3 tuple of n arrays and, optionally, their capacity (left out: the
    second array's rows per window); None: capacity 0 and n NULLs"""
    if rows is None:
        return (0,) + (None,) * n
    return (int(rows[n]) if len(rows) > n else int(rows[1].shape[-2]),) + tuple(_dev(t) for t in rows[:n])


def _host_out(x, dtype, size, optional=False):
    """pointer argument of a host output array: of this dtype, C-contiguous, at least size elements; None only where optional.  (C.cast
    is the cheaper half of ndarray.ctypes.data_as; the pointer does not keep x alive, the caller does.)"""
    if x is None and optional:
        return None
    assert x.dtype == dtype and x.size >= size and x.flags.c_contiguous
    return C.cast(x.ctypes.data, _IP if dtype == _I32 else _DP)


def _dev_out(t, numel, dtype=None, optional=False):
    """pointer argument of a torch output tensor: on the device, contiguous, at least numel elements, of dtype where one is given"""
    if t is None and optional:
        return None
    assert t.is_cuda and t.is_contiguous() and t.numel() >= numel and (dtype is None or t.dtype == dtype)
    return C.c_void_p(t.data_ptr())


class WindowBatch:
    """Host-side arrays of B instances in the ABI's layout; fill with add_* then hand to WindowSolver.solve."""
    TABLES = ("counts", "poses", "r_idx", "r_val", "p_idx", "p_val", "s_idx", "s_val")   # in the C ABI's argument order

    def __init__(self, batch, nv_max, nr_max, np_max, ns_max):
        self.B = int(batch)
        self.caps = (int(nv_max), int(nr_max), int(np_max), int(ns_max))
        self._layout_of = None
        for name, dtype, shape, _ in self._layout():
            setattr(self, name, np.zeros(shape, dtype=dtype))
        self.poses[:, :, 0] = self.poses[:, :, 4] = self.poses[:, :, 8] = 1.0
        self.result = np.zeros((self.B, 8))
        self.r_off1 = None   # optional lever arms of endpoint 1, [B][nr_max][3] (loc_window_set_endpoint1_offsets); created by add_range(off1=...)
        self.p_info = None   # optional full information matrices of the priors, [B][np_max][36] (loc_window_set_prior_information); created by add_prior(info=...)

    def _layout(self):
        """(name, dtype, shape, pointer type) of the eight tables, in TABLES order, for this batch's B and capacities (kept until they change)"""
        if self._layout_of != (self.B, self.caps):
            B, (nv, nr, npr, ns) = self.B, self.caps
            nr, npr, ns = max(nr, 1), max(npr, 1), max(ns, 1)
            rows = ((4,), (nv, 12), (nr, 2), (nr, 5), (npr,), (npr, 18), (ns, 4), (ns, 48))
            self._layout_rows = tuple((name, _F64, (B,) + row, _DP) if k % 2 else (name, _I32, (B,) + row, _IP) for k, (name, row) in enumerate(zip(self.TABLES, rows)))
            self._layout_of = (self.B, self.caps)
        return self._layout_rows

    def _pointers(self):
        """The eight tables as the library takes them: ctypes pointers in TABLES order.  The library sees neither dtypes nor strides, so
        every table is first held to _layout() and to C-contiguity.  The pointers are good for as long as the batch holds these arrays."""
        out = []
        for name, dtype, shape, pointer in self._layout():
            a = getattr(self, name)
            if not (isinstance(a, np.ndarray) and a.dtype == dtype and a.shape == shape and a.flags.c_contiguous):
                what = (f"is a {type(a).__name__}, not a numpy array" if not isinstance(a, np.ndarray) else f"has dtype {a.dtype}, not {dtype}" if a.dtype != dtype
                        else f"has shape {a.shape}, not {shape}" if a.shape != shape else "is not C-contiguous")
                raise ValueError(f"WindowBatch.{name} {what}")
            out.append(C.cast(a.ctypes.data, pointer))
        return out

    def take(self, rows):
        """A new batch of len(rows) windows at the same capacities, window k a copy of this batch's window rows[k]: the eight tables, result,
        and p_info / r_off1 where the batch has them.  Every array is freshly allocated."""
        rows = np.asarray(rows, dtype=np.intp).reshape(-1)
        out = WindowBatch(len(rows), *self.caps)
        for name in self.TABLES + ("result", "p_info", "r_off1"):
            src = getattr(self, name)
            if src is not None:
                dst = np.empty((len(rows),) + src.shape[1:], dtype=src.dtype)
                dst[...] = src[rows]
                setattr(out, name, dst)
        return out

    def copy(self):
        return self.take(np.arange(self.B))

    def tile(self, B):
        """B windows: this batch's windows repeated in order (or its first B)"""
        return self.take(np.arange(B) % self.B)

    def add_pose(self, i, t, R=None):
        v = int(self.counts[i, 0])
        assert v < self.caps[0]
        self.poses[i, v, :9] = (np.eye(3) if R is None else np.asarray(R)).reshape(9)
        self.poses[i, v, 9:] = t
        self.counts[i, 0] = v + 1
        return v

    def add_range(self, i, v0, v1, meas, info, off=(0.0, 0.0, 0.0), anchor=False, off1=None):
        e = int(self.counts[i, 1])
        assert e < self.caps[1]
        self.r_idx[i, e] = (v0, -1 - v1 if anchor else v1)
        self.r_val[i, e] = (meas, info, off[0], off[1], off[2])
        if off1 is not None:
            if self.r_off1 is None:
                self.r_off1 = np.zeros((self.B, max(self.caps[1], 1), 3))
            self.r_off1[i, e] = off1
        self.counts[i, 1] = e + 1

    def add_prior(self, i, v, t, R, info_diag=None, info=None):
        """info_diag: the six diagonal entries; or info: the full symmetric 6x6 (the batch then carries p_info, in which every prior has a
        row: the priors added with info_diag get diag(info_diag))"""
        e = int(self.counts[i, 2])
        assert e < self.caps[2] and (info_diag is None) != (info is None)
        Ri, ti = _inv_iso(np.asarray(R, dtype=float), np.asarray(t, dtype=float))
        self.p_idx[i, e] = v
        if info is not None:
            info = np.asarray(info, dtype=float).reshape(6, 6)
            info_diag = np.diag(info)
            if self.p_info is None:   # the priors so far: their diagonals
                self.p_info = np.zeros((self.B, max(self.caps[2], 1), 36))
                self.p_info[:, :, ::7] = self.p_val[:, :, 12:]
        self.p_val[i, e, :9] = Ri.reshape(9); self.p_val[i, e, 9:12] = ti; self.p_val[i, e, 12:] = info_diag
        if self.p_info is not None:
            self.p_info[i, e] = (np.diag(np.asarray(info_diag, dtype=float)) if info is None else info).reshape(36)
        self.counts[i, 2] = e + 1

    def add_se3(self, i, vi, vj, t, R, info, robust=True):
        e = int(self.counts[i, 3])
        assert e < self.caps[3]
        Ri, ti = _inv_iso(np.asarray(R, dtype=float), np.asarray(t, dtype=float))
        self.s_idx[i, e] = (vi, vj, int(robust), 0)
        self.s_val[i, e, :9] = Ri.reshape(9); self.s_val[i, e, 9:12] = ti
        self.s_val[i, e, 12:] = np.asarray(info, dtype=float).reshape(36)
        self.counts[i, 3] = e + 1

    def pose(self, i, v):
        return self.poses[i, v, :9].reshape(3, 3).copy(), self.poses[i, v, 9:].copy()


def covariance_plan(wb: WindowBatch):
    """(blocks_max, workspace_bytes) of loc_window_covariance_plan: the largest envelope of wb's windows in 6x6 blocks, in their pose
    order, and the device workspace the envelope pass (option "covariance_general") allocates for the batch.  Host only: no device."""
    caps = WindowCaps(*wb.caps, -1)
    counts, _, r_idx, _, _, _, s_idx, _ = wb._pointers()
    blocks, nbytes = C.c_int64(), C.c_size_t()
    check(lib().loc_window_covariance_plan(C.byref(caps), wb.B, counts, r_idx, s_idx, C.byref(blocks), C.byref(nbytes)))
    return blocks.value, nbytes.value


def _pair_tables(B, pairs, pair_counts):
    """(npair_max, pair_counts int32 [B], pairs int32 [B][npair_max][2]) as the joint covariance calls take them.  pairs: [B][npair_max][2],
    or [npair_max][2] for every window alike; pair_counts None: every window has all npair_max pairs.  Nothing is checked here: the
    library validates every count and slot."""
    pairs = np.asarray(pairs, dtype=np.int32)
    if pairs.ndim == 2:
        pairs = np.broadcast_to(pairs, (B,) + pairs.shape)
    assert pairs.ndim == 3 and pairs.shape[0] == B and pairs.shape[2] == 2
    pairs = np.ascontiguousarray(pairs)
    npm = pairs.shape[1]
    pair_counts = np.full(B, npm, dtype=np.int32) if pair_counts is None else np.ascontiguousarray(pair_counts, dtype=np.int32).reshape(B)
    return npm, pair_counts, pairs


def joint_covariance_plan(wb: WindowBatch, pairs, pair_counts=None):
    """covariance_plan(wb) for a joint call: the envelope pass keeps [H^-1]_ij of a requested pair in the block that pair adds to the envelope
    (loc_window_joint_covariance_plan).  Without pairs: covariance_plan(wb)."""
    caps = WindowCaps(*wb.caps, -1)
    counts, _, r_idx, _, _, _, s_idx, _ = wb._pointers()
    npm, pc, pr = _pair_tables(wb.B, pairs, pair_counts)
    blocks, nbytes = C.c_int64(), C.c_size_t()
    check(lib().loc_window_joint_covariance_plan(C.byref(caps), wb.B, counts, r_idx, s_idx, npm, pc.ctypes.data_as(_IP), pr.ctypes.data_as(_IP),
                                                 C.byref(blocks), C.byref(nbytes)))
    return blocks.value, nbytes.value


class WindowSolver(_lib.Handle):
    _prefix = "loc_window"

    def __init__(self, anchors, batch, nv_max, nr_max, np_max=0, ns_max=0, maximum_iteration=10, device=0, bw_max=-1,
                 jacobian="numeric", natural_order=False, chain_threshold=None):
        L = lib()
        if L.loc_device_count() <= 0:
            raise _lib.LocalizationAmdError(_lib.LOC_ERR_NO_DEVICE, "no HIP device visible: localization_amd has no CPU fallback")
        anchors = np.ascontiguousarray(anchors, dtype=np.float64).reshape(-1, 3)
        caps = WindowCaps(nv_max, nr_max, np_max, ns_max, bw_max)
        h = C.c_void_p()
        check(L.loc_window_create(C.byref(h), device, int(batch), C.byref(caps), anchors.shape[0],
                                  anchors.ctypes.data_as(C.POINTER(C.c_double)), int(maximum_iteration)))
        self.h, self.L, self.B = h, L, int(batch)
        self._resident = 0   # windows of the resident batch (upload / upload_dev)
        self.caps = (nv_max, nr_max, np_max, ns_max)
        self.lds_bytes = L.loc_window_lds_bytes(C.byref(caps))
        check(L.loc_window_set_jacobian(h, _lib.JAC_NUMERIC_G2O if jacobian in ("numeric", _lib.JAC_NUMERIC_G2O) else _lib.JAC_ANALYTIC))
        check(L.loc_window_set_ordering(h, int(bool(natural_order))))
        if chain_threshold is not None:   # smallest batch that takes the one-lane-per-window kernel for chain windows
            check(L.loc_window_set_chain_threshold(h, int(chain_threshold)))

    def _endpoint1(self, wb):
        check(self.L.loc_window_set_endpoint1_offsets(self.h, wb.B, None if wb.r_off1 is None else np.ascontiguousarray(wb.r_off1).ctypes.data_as(_DP)))

    def _prior_information(self, wb):
        check(self.L.loc_window_set_prior_information(self.h, wb.B, None if wb.p_info is None else np.ascontiguousarray(wb.p_info, dtype=np.float64).ctypes.data_as(_DP)))

    def _tables(self, wb, refuse_off1=None):
        """wb's eight table pointers (checked before any library call), after its prior table and its endpoint-1 lever arms are handed to
        the handle.  refuse_off1: the name of a call that does not serve lever arms; it refuses them and leaves the handle's as they are."""
        assert wb.caps == self.caps and wb.B <= self.B
        tables = wb._pointers()
        if refuse_off1 is None:
            self._endpoint1(wb)
        elif wb.r_off1 is not None:   # (the handle's endpoint-1 lever arms belong to its solves and stay as they are)
            raise _lib.LocalizationAmdError(-5, f"{refuse_off1}: windows with endpoint-1 lever arms are not supported")
        self._prior_information(wb)
        return tables

    def solve(self, wb: WindowBatch):
        tables = self._tables(wb)
        check(self.L.loc_window_solve_host(self.h, wb.B, *tables, _host_out(wb.result, _F64, wb.B * 8)))
        return wb.result

    # ---- device-resident operation: upload once, solve any number of times from the uploaded estimates, download
    def upload(self, wb: WindowBatch):
        check(self.L.loc_window_upload(self.h, wb.B, *self._tables(wb)))
        self._resident = wb.B

    def upload_dev(self, counts, poses, r_idx, r_val, p_idx, p_val, s_idx, s_val, n=None, admit=None, stream=None):
        """upload() from device memory (loc_window_upload_dev): the eight tables in upload()'s layouts at the handle's capacities — counts int32
        [n][4], poses float64 [n][nv_max][12], r_idx int32 [n][nr_max][2], r_val float64 [n][nr_max][5], p_idx int32 [n][np_max], p_val float64
        [n][np_max][18], s_idx int32 [n][ns_max][4], s_val float64 [n][ns_max][48] — each a device pointer, an object with data_ptr() or None (a
        table under a capacity of 0).  n: the windows (None: counts.shape[0]).  admit: int32 [n] on the device or None; window b's code (0
        admitted, 1 .. 6 the check it fails).  Every window is admitted and the chain family's structure scanned by a HIP pass on stream (a torch
        stream; None: the handle's own; set_option("upload_dev_structures", 1): the arrowhead and forest verdicts as well; with
        set_option("upload_dev_forest_groups", 1) and set_option("forest_groups", 1) also the groups of a mixed forest batch); a batch with a refused window raises (LOC_ERR_INVALID; the error names the check and the lowest refused
        window) and leaves the previous resident batch as it was.  Returns when the arrays are free again, like upload().  The handle's tables of
        endpoint-1 lever arms / full information matrices stay as they are.  Plumbing only: the library checks everything."""
        n = int(counts.shape[0]) if n is None else int(n)
        check(self.L.loc_window_upload_dev(self.h, _stream(stream), n, *(_dev(t) for t in (counts, poses, r_idx, r_val, p_idx, p_val, s_idx, s_val)), _dev(admit)))
        self._resident = n

    def solve_resident(self, stream=None):
        check(self.L.loc_window_solve_resident(self.h, stream))

    def download(self, wb: WindowBatch):
        check(self.L.loc_window_download(self.h, wb.poses.ctypes.data_as(_DP), wb.result.ctypes.data_as(_DP)))
        return wb.result

    def _covariance_out(self, B, out, npm=None):
        """(cov, mask, status[, cross]) of a covariance call on B windows, the caller's or fresh, and their pointer arguments"""
        nv = self.caps[0]
        if out is None:
            out = (np.zeros((B, nv, 6, 6)), np.zeros((B, nv), dtype=np.int32), np.zeros(B, dtype=np.int32)) + (() if npm is None else (np.zeros((B, npm, 6, 6)),))
        sizes = ((_F64, B * nv * 36), (_I32, B * nv), (_I32, B)) + (() if npm is None else ((_F64, B * npm * 36),))
        return tuple(out), [_host_out(x, dt, size) for x, (dt, size) in zip(out, sizes, strict=True)]

    # ---- marginal pose covariances at the given (solved) estimates (loc_window_covariance_*)
    def covariance(self, wb: WindowBatch, out=None):
        """Sigma_i = [H^-1]_ii of every pose of every window at wb.poses: chain windows of <= 64 poses, arrowhead batches (anchor
        self-calibration; the unknown anchors are the last pose slots) whenever the handle would solve them on arrow3_lm_kernel (option
        "arrow3"; by default handles of more than 64 poses), and forest batches (one shared topology, <= 64 poses) whenever the handle
        would solve them on a forest kernel (option "tree", batch threshold); forest batches of DIFFERING topologies under options
        "forest_groups" + "forest_groups_covariance"; with set_option("covariance_general", 1) any other batch
        as well, on the envelope pass in the caller's pose order (covariance_plan reports its memory).  Returns (cov [B][nv_max][6][6],
        mask [B][nv_max] — excluded coordinates, bits 0-5 = tx ty tz qx qy qz —, status [B]: 0 or LOC_ERR_SINGULAR, that window's blocks NaN).
        The C call is stateless; THIS method first hands wb's prior table to the handle (_prior_information: wb.p_info, or none), as
        solve() and upload() do, and so do joint_covariance() and marginal_prior().  The table belongs to the handle, not to a batch: after
        upload(batch with p_info) a covariance(another batch without one) clears it, and the resident batch is from then on solved and
        served with p_val's diagonals until a call with the table sets it again.  (The endpoint-1 lever arms are never touched here.)"""
        tables = self._tables(wb, refuse_off1="covariance")
        out, args = self._covariance_out(wb.B, out)   # (out: caller's arrays of these shapes and dtypes; left untouched when the call fails)
        check(self.L.loc_window_covariance_host(self.h, wb.B, *tables, *args))
        return out

    # ---- the marginal prior of a dropped pose (loc_window_marginal_prior_host)
    def marginal_prior(self, wb: WindowBatch, drop, out=None):
        """What dropping pose drop[b] of every (translation-only) window leaves on its one neighbour, at wb.poses: returns (slot [B] — the
        neighbour, -1: none —, prior [B][48] — Z^-1 as R(9), t(3) and the 6x6 information: add_prior's row —, grad [B][6], shift [B][6],
        rank [B], status [B]: 0 or LOC_ERR_SINGULAR, then a zero-information row = the plain drop).  drop: int [B], or one slot for all."""
        tables = self._tables(wb, refuse_off1="marginal_prior")
        drop = np.ascontiguousarray(np.broadcast_to(np.asarray(drop, dtype=np.int32), (wb.B,)))
        if out is None:
            out = (np.zeros(wb.B, dtype=np.int32), np.zeros((wb.B, 48)), np.zeros((wb.B, 6)), np.zeros((wb.B, 6)), np.zeros(wb.B, dtype=np.int32),
                   np.zeros(wb.B, dtype=np.int32))
        slot, prior, grad, shift, rank, status = out   # (out: caller's arrays of these shapes and dtypes; left untouched when the call fails)
        args = [_host_out(x, dt, wb.B * width) for x, dt, width in ((slot, _I32, 1), (prior, _F64, 48), (grad, _F64, 6), (shift, _F64, 6), (rank, _I32, 1),
                                                                    (status, _I32, 1))]
        check(self.L.loc_window_marginal_prior_host(self.h, wb.B, *tables, drop.ctypes.data_as(_IP), *args))
        return slot, prior, grad, shift, rank, status

    def covariance_resident(self, cov, mask, status, stream=None):
        """The same for the uploaded batch at its solved poses (after solve_resident), asynchronous, into torch device tensors: cov float64
        [B][nv_max][6][6] (or [..][36]), mask int32 [B][nv_max], status int32 [B].  stream: a torch stream (None: the handle's own stream)."""
        import torch
        n = self._resident
        args = [_dev_out(t, numel, dt) for t, dt, numel in ((cov, torch.float64, n * self.caps[0] * 36), (mask, torch.int32, n * self.caps[0]), (status, torch.int32, n))]
        check(self.L.loc_window_covariance_resident(self.h, _stream(stream), *args))

    # ---- the resident fixed-lag slide (loc_window_slide_resident / loc_window_download_tables; DESIGN.md §2, "The resident slide")
    def slide_resident(self, new_pose, new_ranges=None, new_priors=None, drop_oldest=None, out=None, stream=None):
        """Slide every uploaded window on the device (after set_option("resident_slide", 1), upload() and solve_resident()): drop slot 0 and
        carry its marginal prior, append new_pose [B][12] (R(9), t(3)) with its factors.  new_ranges: (counts int [B], r_idx int
        [B][nr_new_max][2], r_val [B][nr_new_max][5]) in the NEW window's numbering; new_priors: (counts int [B], p_val [B][np_new_max][18]) on the
        new pose, or None; drop_oldest: int [B] (0: that window only grows), None: every window drops.  out: (slot, prior, rank, status) torch
        device tensors (int32 [B], float64 [B][48], int32 [B], int32 [B]), each may be None.  Asynchronous on stream (a torch stream; None: the
        handle's own); the numpy inputs are read before the call returns.  Plumbing only: the library checks everything."""
        n = self._resident
        pose = np.ascontiguousarray(new_pose, dtype=np.float64).reshape(n, 12)
        drop = None if drop_oldest is None else np.ascontiguousarray(np.broadcast_to(np.asarray(drop_oldest, dtype=np.int32), (n,)))
        r_args = (0, None, None, None)
        if new_ranges is not None:   # (the arrays converted here stay alive until the call has read them)
            rc = np.ascontiguousarray(new_ranges[0], dtype=np.int32).reshape(n)
            ri = np.ascontiguousarray(new_ranges[1], dtype=np.int32).reshape(n, -1, 2)
            rv = np.ascontiguousarray(new_ranges[2], dtype=np.float64).reshape(n, ri.shape[1], 5)
            r_args = (ri.shape[1], rc.ctypes.data_as(_IP), ri.ctypes.data_as(_IP), rv.ctypes.data_as(_DP))
        p_args = (0, None, None)
        if new_priors is not None:
            pc = np.ascontiguousarray(new_priors[0], dtype=np.int32).reshape(n)
            pv = np.ascontiguousarray(new_priors[1], dtype=np.float64).reshape(n, -1, 18)
            p_args = (pv.shape[1], pc.ctypes.data_as(_IP), pv.ctypes.data_as(_DP))
        outs = [_dev_out(t, numel, optional=True) for t, numel in zip(out if out is not None else (None,) * 4, (n, n * 48, n, n))]
        check(self.L.loc_window_slide_resident(self.h, _stream(stream), None if drop is None else drop.ctypes.data_as(_IP), pose.ctypes.data_as(_DP),
                                               *r_args, *p_args, *outs))

    def slide_resident_dev(self, new_pose, new_ranges, new_priors=None, drop_oldest=None, out=None, stream=None):
        """slide_resident() with every per-window input in device memory (loc_window_slide_resident_dev): device pointers (int) or objects
        with data_ptr(), in slide_resident()'s layouts — new_pose float64 [B][12]; new_ranges (counts int32 [B], r_idx int32 [B][nr_new_max][2],
        r_val float64 [B][nr_new_max][5], nr_new_max) or None; new_priors (counts int32 [B], p_val float64 [B][np_new_max][18], np_new_max) or
        None; drop_oldest int32 [B] or None (every window drops).  The capacities may be left out for objects with a shape.  out: (slot, prior,
        rank, status, admit), each a device pointer, an object with data_ptr() or None.  Each wave admits its own window: admit[b] is 0 or the
        code of the rule window b breaks, and a refused window stays as it was.  Asynchronous on stream (a torch stream; None: the handle's own),
        no host pass, no copy: the caller keeps the arrays alive and unchanged until the stream has passed the call, and orders its own writes to
        them before it.  Plumbing only: the library checks everything."""
        outs = [_dev(t) for t in (out if out is not None else (None,) * 5)]
        check(self.L.loc_window_slide_resident_dev(self.h, _stream(stream), _dev(drop_oldest), _dev(new_pose), *_new_rows(new_ranges, 3),
                                                   *_new_rows(new_priors, 2), *outs))

    def slide_plain_resident_dev(self, new_pose, new_ranges, new_priors=None, new_se3=None, drop_oldest=None, out=None, stream=None):
        """The plain drop for resident 6-DoF chain batches (loc_window_slide_plain_resident_dev): slot 0 goes with every factor on it, nothing
        is carried, new_pose and its factors are appended.  Every per-window input is in device memory, as for slide_resident_dev(): new_pose
        float64 [B][12] (any rotation); new_ranges (counts int32 [B], r_idx int32 [B][nr_new_max][2], r_val float64 [B][nr_new_max][5],
        nr_new_max) or None; new_priors (counts int32 [B], p_val float64 [B][np_new_max][18], np_new_max) or None; new_se3 (counts int32 [B],
        s_idx int32 [B][ns_new_max][4], s_val float64 [B][ns_new_max][48], ns_new_max) or None; drop_oldest int32 [B] or None (every window
        drops).  The capacities may be left out for objects with a shape.  out: (status, admit), each a device pointer, an object with
        data_ptr() or None.  Each wave admits its own window: admit[b] is 0 or the code of the rule window b breaks, and a refused window stays
        as it was.  Asynchronous on stream (a torch stream; None: the handle's own), no host pass, no copy: the caller keeps the arrays alive
        and unchanged until the stream has passed the call.  Plumbing only: the library checks everything."""
        outs = [_dev(t) for t in (out if out is not None else (None,) * 2)]
        check(self.L.loc_window_slide_plain_resident_dev(self.h, _stream(stream), _dev(drop_oldest), _dev(new_pose), *_new_rows(new_ranges, 3),
                                                         *_new_rows(new_priors, 2), *_new_rows(new_se3, 3), *outs))

    # ---- rows from raw messages (loc_window_set_message_config / _message_rows_dev / _push_messages_resident_dev)
    MSG_RANGE, MSG_IMU, MSG_LIDAR, MSG_TWIST = 1, 2, 4, 8
    MSG_NONE, MSG_APPENDED, MSG_REJECTED, MSG_INVALID, MSG_SINGULAR = 0, 1, 2, 3, 4
    MSG_FIELDS = ("kind", "dt", "anchor", "antenna", "distance", "distance_err", "imu", "lidar_z", "twist")
    MSG_ROWS = ("drop_oldest", "new_pose", "new_r_counts", "new_r_idx", "new_r_val", "new_p_counts", "new_p_val", "new_s_counts", "new_s_idx",
                "new_s_val", "verdict")

    def set_message_config(self, trajectory_length, maximum_velocity=1.0, distance_outlier=1.0, antenna_xyz=None):
        """The configuration the message calls read (the reference's robot/trajectory_length, maximum_velocity, distance_outlier — <= 0: no
        gate — and /uwb/antennaOffset as [n_antenna][3]); also allocates the handle's block of output arrays."""
        cfg = MessageConfig(int(trajectory_length), float(maximum_velocity), float(distance_outlier))
        ant = None if antenna_xyz is None else np.ascontiguousarray(antenna_xyz, dtype=np.float64).reshape(-1, 3)
        check(self.L.loc_window_set_message_config(self.h, C.byref(cfg), 0 if ant is None else ant.shape[0], None if ant is None else ant.ctypes.data_as(_DP)))

    @staticmethod
    def _ptr_struct(fields, values):
        """a struct of len(fields) void pointers from a dict of device pointers (int) or objects with data_ptr(); a missing name is NULL"""
        return (C.c_void_p * len(fields))(*[_dev(values.get(f)).value for f in fields])

    def message_rows_dev(self, kinds_mask, msgs, out, stream=None):
        """Build only (loc_window_message_rows_dev): msgs a dict of the message arrays by MSG_FIELDS' names (kind int32 [B], dt float64 [B],
        anchor / antenna int32 [B], distance / distance_err float32 [B], imu float64 [B][7], lidar_z float64 [B], twist float64 [B][42]), out
        a dict of the eleven output arrays by MSG_ROWS' names ("verdict" may be missing); device pointers or objects with data_ptr().
        Asynchronous on stream (a torch stream; None: the handle's own).  Plumbing only: the library checks everything."""
        m, o = self._ptr_struct(self.MSG_FIELDS, msgs), self._ptr_struct(self.MSG_ROWS, out)
        check(self.L.loc_window_message_rows_dev(self.h, _stream(stream), int(kinds_mask), C.byref(m), C.byref(o)))

    def push_messages_resident_dev(self, kinds_mask, msgs, verdict=None, status=None, admit=None, stream=None):
        """Build into the handle's own block, then the slide the resident verdict calls for, on the same stream
        (loc_window_push_messages_resident_dev).  msgs as for message_rows_dev(); verdict / status / admit int32 [B] device arrays or None.
        Read verdict first: a window with MSG_NONE or MSG_REJECTED shows admit code 2, and that is not an error."""
        m = self._ptr_struct(self.MSG_FIELDS, msgs)
        check(self.L.loc_window_push_messages_resident_dev(self.h, _stream(stream), int(kinds_mask), C.byref(m), _dev(verdict), _dev(status), _dev(admit)))

    def download_batch(self):
        """The resident batch as it stands, as a WindowBatch (loc_window_download_tables): counts, the estimates the next resident solve
        starts from, every index and value table, and p_info when the handle has a table of full information matrices."""
        wb = WindowBatch(self._resident, *self.caps)
        check(self.L.loc_window_download_tables(self.h, *wb._pointers(), None))
        pinfo = np.zeros((wb.B, max(self.caps[2], 1), 36))
        if self.L.loc_window_download_tables(self.h, None, None, None, None, None, None, None, None, pinfo.ctypes.data_as(_DP)) == _lib.LOC_OK:
            wb.p_info = pinfo   # (LOC_ERR_INVALID: the handle has no table)
        return wb

    # ---- the per-edge chi2 audit and the reference's outlier-range removal (loc_window_edge_chi2_* / loc_window_prune_resident)
    def edge_chi2(self, wb: WindowBatch, out=None):
        """chi2 = e^T Omega e (not robustified) of every edge of every window at wb.poses, any structure: returns (r_chi2 [B][nr_max], p_chi2
        [B][np_max], s_chi2 [B][ns_max] — slots beyond a window's count 0 —, total [B], active int32 [B] = range rows with information != 0
        + priors + EdgeSE3).  out: the caller's five arrays, each may be None (that output is skipped).  Hands wb's endpoint-1 lever arms and
        prior table to the handle first, as solve() does."""
        tables = self._tables(wb)
        if out is None:
            out = (np.zeros((wb.B, max(self.caps[1], 1))), np.zeros((wb.B, max(self.caps[2], 1))), np.zeros((wb.B, max(self.caps[3], 1))),
                   np.zeros(wb.B), np.zeros(wb.B, dtype=np.int32))
        args = [_host_out(x, dt, wb.B * width, optional=True) for x, dt, width in zip(out, (_F64,) * 4 + (_I32,), self.caps[1:] + (1, 1), strict=True)]
        check(self.L.loc_window_edge_chi2_host(self.h, wb.B, *tables, *args))
        return tuple(out)

    def edge_chi2_resident(self, r_chi2, p_chi2, s_chi2, total, active, stream=None):
        """The same for the uploaded batch at its solved poses (after solve_resident), asynchronous, into torch device tensors (float64
        [B][nr_max] / [B][np_max] / [B][ns_max] / [B], int32 [B]); each may be None.  stream: a torch stream (None: the handle's own)."""
        n = self._resident
        args = [_dev_out(t, n * width, optional=True) for t, width in zip((r_chi2, p_chi2, s_chi2, total, active), self.caps[1:] + (1, 1))]
        check(self.L.loc_window_edge_chi2_resident(self.h, _stream(stream), *args))

    def prune_resident(self, chi2_max=2.0, min_edges=100, removed=None, n_removed=None, stream=None):
        """The reference's removal rule on the uploaded batch, in place on the device (after solve_resident): a window with more than min_edges
        active edges gets information 0.0 on every range row with information != 0 and chi2 > chi2_max at the solved poses.  removed int32
        [B][nr_max], n_removed int32 [B]: torch device tensors, each may be None.  Asynchronous on stream (None: the handle's own)."""
        n = self._resident
        args = [_dev_out(t, numel, optional=True) for t, numel in ((removed, n * self.caps[1]), (n_removed, n))]
        check(self.L.loc_window_prune_resident(self.h, _stream(stream), float(chi2_max), int(min_edges), *args))

    # ---- publish and path records of the resident batch (loc_window_publish_resident / loc_window_path_resident)
    def publish_resident(self, minimum_optimize_error, trajectory_length, flags, realtime=None, optimized=None, chi2=None, n_published=None, stream=None):
        """The reference's publish step for the uploaded batch (after solve_resident), on the device: flags int32 [B] (bit 0: chi2 <
        minimum_optimize_error and the window has a pose; bit 1: path index trajectory_length // 2 is in the window), realtime / optimized
        float64 [B][7] (x, y, z, qx, qy, qz, qw; written only with bit 0 / bits 0 and 1), chi2 float64 [B], n_published int32 [1].  Device
        pointers or objects with data_ptr(); all but flags may be None.  Asynchronous on stream (a torch stream; None: the handle's own).
        Plumbing only: the library checks everything."""
        check(self.L.loc_window_publish_resident(self.h, _stream(stream), float(minimum_optimize_error), int(trajectory_length), _dev(flags), _dev(realtime),
                                                 _dev(optimized), _dev(chi2), _dev(n_published)))

    def path_resident(self, trajectory_length, path, present, first=0, count=None, stream=None):
        """Path indices first .. first + count - 1 (count None: up to trajectory_length - 1) of every window of the uploaded batch: path float64
        [B][count][7], written only where present int32 [B][count] is 1.  first = 0: vertices2path; first = trajectory_length // 2: the tail
        the reference flushes at exit.  Device pointers or objects with data_ptr().  Asynchronous on stream; plumbing only."""
        count = int(trajectory_length) - int(first) if count is None else int(count)
        check(self.L.loc_window_path_resident(self.h, _stream(stream), int(trajectory_length), int(first), count, _dev(path), _dev(present)))

    def covariance_plan(self, wb: WindowBatch):
        """covariance_plan(wb) for this handle's capacities"""
        assert wb.caps == self.caps
        return covariance_plan(wb)

    # ---- joint marginals: covariance() and the cross blocks [H^-1]_ij of requested pose pairs (loc_window_joint_covariance_*)
    def joint_covariance(self, wb: WindowBatch, pairs, pair_counts=None, out=None):
        """covariance(wb) and cross [B][npair_max][6][6]: cross[b][p] = [H^-1]_ij for pair p = (i, j) of window b (rows: pose i's
        coordinates; excluded rows / columns 0; NaN for a singular window; slots p >= pair_counts[b] are 0).  pairs: int [B][npair_max][2]
        pose slots, or [npair_max][2] for every window alike; pair_counts: [B], None = all of them.  Same coverage as covariance(); a pair
        count or a slot out of range raises LOC_ERR_INVALID with nothing written.  Returns (cov, mask, status, cross)."""
        tables = self._tables(wb, refuse_off1="covariance")
        npm, pc, pr = _pair_tables(wb.B, pairs, pair_counts)
        out, args = self._covariance_out(wb.B, out, npm)   # (out: caller's arrays of these shapes and dtypes; left untouched when the call fails)
        check(self.L.loc_window_joint_covariance_host(self.h, wb.B, *tables, npm, pc.ctypes.data_as(_IP), pr.ctypes.data_as(_IP), *args))
        return out

    def joint_covariance_resident(self, pairs, pair_counts, cov, mask, status, cross, stream=None):
        """joint_covariance for the uploaded batch at its solved poses, asynchronous: pairs / pair_counts numpy arrays as above (read before
        the call returns), cov / mask / status / cross torch device tensors (cross float64 [B][npair_max][6][6] or [..][36])."""
        import torch
        n = self._resident
        npm, pc, pr = _pair_tables(n, pairs, pair_counts)
        args = [_dev_out(t, numel, dt) for t, dt, numel in ((cov, torch.float64, n * self.caps[0] * 36), (mask, torch.int32, n * self.caps[0]), (status, torch.int32, n),
                                                            (cross, torch.float64, n * npm * 36))]
        check(self.L.loc_window_joint_covariance_resident(self.h, _stream(stream), npm, pc.ctypes.data_as(_IP), pr.ctypes.data_as(_IP), *args))

    def joint_covariance_plan(self, wb: WindowBatch, pairs, pair_counts=None):
        """joint_covariance_plan(wb, pairs, pair_counts) for this handle's capacities"""
        assert wb.caps == self.caps
        return joint_covariance_plan(wb, pairs, pair_counts)

    def last_covariance_ms(self):
        ms = C.c_double()
        check(self.L.loc_window_last_covariance_ms(self.h, C.byref(ms)))
        return ms.value

    COVARIANCE_KINDS = {0: "none", 1: "covariance_kernel<3>", 2: "covariance_kernel<6>", 3: "arrow_covariance_kernel", 4: "forest_covariance_kernel",
                        5: "envelope_covariance_kernel", 6: "forest_covariance_kernel<groups>"}

    def last_covariance_kind(self):
        """name of the pass that served the last covariance() / joint_covariance() / *_resident() call that launched
        (loc_window_last_covariance_kind); "none" before the first"""
        k = C.c_int32()
        check(self.L.loc_window_last_covariance_kind(self.h, C.byref(k)))
        return self.COVARIANCE_KINDS.get(k.value, str(k.value))

    KERNEL_KINDS = {-1: "none", 0: "window_lm_kernel", 1: "chain_lm_kernel", 2: "chain3_lm_kernel", 3: "arrow3_lm_kernel", 4: "tree_wave_kernel", 5: "tree_lm_kernel", 6: "wave3_lm_kernel", 7: "wave6_lm_kernel", 8: "wave6_lm_kernel<SE3>",
                    9: "tree_wave_kernel<groups>"}

    def last_kernel_kind(self):
        """name of the kernel the last solve ran (loc_window_last_kernel_kind)"""
        k = C.c_int32()
        check(self.L.loc_window_last_kernel_kind(self.h, C.byref(k)))
        return self.KERNEL_KINDS.get(k.value, str(k.value))

    def last_kernel_ms(self):
        ms = C.c_double()
        check(self.L.loc_window_last_kernel_ms(self.h, C.byref(ms)))
        return ms.value

    def set_option(self, name, value):
        """loc_window_set_option: the kernel-selection switches of this handle ("chain_min_batch", "arrow3", "tree", "wave3", "wave6",
        "chain3", "zero_copy", "topology_cache", "kernel_events"; "resident_slide": 1 = upload() keeps what slide_resident() needs, default 0;
        "covariance_general": 1 = covariance() / covariance_resident() also serve
        the batches the chain, arrowhead and forest passes decline — every batch with full-information priors among them —, default 0;
        "prior_information_structured": 1 = a translation-only p_info table (dense 3 x 3 blocks on the translations: marginal_prior()'s rows)
        on translation-only chains of <= 64 poses is solved by wave3_lm_kernel and served by the chain 3 x 3 covariance pass, default 0;
        "upload_dev_structures": 1 = upload_dev() also takes the arrowhead and forest verdicts on the device, so that such a batch runs on
        arrow3_lm_kernel / tree_wave_kernel and its covariance passes exactly as after upload() of the same arrays; default 0: a batch
        uploaded from device arrays that is no chain solves on the general kernel;
        "forest_groups": 1 = a batch of forest windows of <= 64 poses whose topologies differ (other parents, lengths, anchors: key-frame windows
        of different robots or phases) is grouped by topology and solved by tree_wave_kernel<groups> with one schedule per group, from solve()
        and from upload() + solve_resident(); a one-topology batch keeps tree_wave_kernel; upload_dev() groups only under "upload_dev_forest_groups", and covariances of a
        mixed batch are served as without the option; default 0: such a batch solves on the general kernel;
        "upload_dev_forest_groups": 1 (with "upload_dev_structures" and "forest_groups" 1) = upload_dev() groups such a mixed batch by topology
        on the device and leaves the handle as upload() of the same arrays does — tree_wave_kernel<groups>, the same forest_groups(), the grouped
        covariance pass on the uploaded block; default 0: a mixed batch in device arrays solves on the general kernel;
        "upload_dev_groups_hash_bits": 0 .. 64, default 64 — a TEST SEAM: that pass's candidate hash keeps this many low bits (fewer bits force
        hash collisions; the answer does not change);
        "forest_groups_covariance": 1 (with "forest_groups" 1) = the covariances and cross blocks of such a mixed batch are computed by
        forest_covariance_kernel<groups>, one wave per window on its group's schedule, from covariance() / joint_covariance() and their
        resident forms; default 0: the envelope pass under "covariance_general", else unsupported)"""
        check(self.L.loc_window_set_option(self.h, str(name).encode(), int(value)))

    def forest_groups(self):
        """(number of topology groups, bytes of schedule tables sent to the device) of the handle's last structural verdict — solve() or
        upload() / upload_dev(), whichever came last; (0, 0) when that batch is not on the grouped path (option "forest_groups")"""
        n, nbytes = C.c_int32(), C.c_int64()
        check(self.L.loc_window_forest_groups(self.h, C.byref(n), C.byref(nbytes)))
        return int(n.value), int(nbytes.value)

    def last_host_timing(self):
        """(validate ms, structure analysis ms, staging + launch + copy back ms, verdict came from the cache) of the last solve()"""
        t = (C.c_double * 4)()
        check(self.L.loc_window_last_host_timing(self.h, t))
        return float(t[0]), float(t[1]), float(t[2]), bool(t[3])
