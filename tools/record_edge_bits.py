#!/usr/bin/env python3
"""Bit records of every kernel that linearises the 6-DoF range, prior and EdgeSE3 factors (localization_amd/csrc/se3_edge_device.h).

    tools/record_edge_bits.py LIBRARY.so OUT.npz

runs the cases below on LIBRARY (any build of liblocalization_amd.so: the golden file tests/golden/edge_terms_parent_bits.npz was recorded
with the library of the commit BEFORE any of the factors was shared through that header) from seeded inputs and writes inputs and outputs to one
np.savez_compressed file, doubles as uint64.  Every case runs twice; a case whose two runs differ in any bit is left out and named on
stdout (exit status 2).  tests/test_gpu_edge_terms_bits.py runs the same cases on the built library and requires every array to be equal.

Arrays of more than FULL_BYTES are kept as one 64-bit digest per window (the first 8 bytes of the sha256 of the window's bytes; key suffix
"#rows"): one flipped bit anywhere changes the digest, and the file stays small (64 windows of 40 poses are 245 KB of estimates alone).
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_BYTES = 2048
ANCH = np.array([[3, -3, 0.58], [3, 3, 1.97], [-3, 3, 0.54], [-3, -3, 1.76]], dtype=float)
OFF = np.array([0.1, 0.0, -0.05])
IMU_INFO = np.array([0, 0, 0, 1, 1, 1.0]) / 4.592449e-06
RANGE_INFO, SMOOTH_INFO = 1 / 0.055 ** 2, 1 / (5.0 / 32 / 3) ** 2
GENERAL, LANES = {"chain_min_batch": 0}, {"chain_min_batch": 1}


def rotvec(v):
    th = float(np.linalg.norm(v))
    if th == 0.0:
        return np.eye(3)
    k = np.asarray(v) / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def windows(la, seed, B, T, se3=None, all_anchors=False, pinfo=False, off1=False, every=4):
    """B windows of T 6-DoF poses: anchor ranges with a lever arm (one per pose, or all four), a smoothness range between consecutive poses,
    an IMU prior on every pose; se3 = "keys": an EdgeSE3 from each pose's key frame (a new key every `every` poses; the pose before a new key
    IS that key, so its smoothness range shares the pair), "forest": the same without the smoothness ranges that would close a cycle,
    "twist": an EdgeSE3 between consecutive poses.  pinfo: full 6x6 information on the priors; off1: lever arms on endpoint 1 of every range.
    The extras draw from generators of their own: the twins share every other number."""
    rng, rng_w, rng_o = np.random.default_rng(seed), np.random.default_rng(seed + 1), np.random.default_rng(seed + 2)
    wb = la.WindowBatch(B, T, 5 * T if all_anchors else 2 * T, T, T if se3 else 0)
    key = np.where(np.arange(T) < every, 0, (np.arange(T) // every) * every - 1)
    for i in range(B):
        tt = np.cumsum(rng.normal(0, 0.05, (T, 3)), axis=0) + np.array([rng.uniform(-1.5, 1.5), rng.uniform(-1.5, 1.5), 1.1])
        rv = np.cumsum(rng.normal(0, 0.03, (T, 3)), axis=0) + rng.normal(0, 0.3, 3)
        tR = np.array([rotvec(r) for r in rv])
        for k in range(T):
            wb.add_pose(i, tt[k] + rng.normal(0, 0.05, 3), tR[k] @ rotvec(rng.normal(0, 0.02, 3)))
        for k in range(T):
            for a in (range(4) if all_anchors else (k % 4,)):
                o1 = rng_o.normal(0, 0.05, 3) if off1 else None
                d = np.linalg.norm(tt[k] + tR[k] @ OFF - ANCH[a] - (o1 if off1 else 0.0))
                wb.add_range(i, k, a, float(np.float32(d + rng.normal(0, 0.03))), RANGE_INFO, OFF, anchor=True, off1=o1)
            if k > 0 and (se3 != "forest" or key[k] == k - 1):
                wb.add_range(i, k - 1, k, 0.0, SMOOTH_INFO, off1=rng_o.normal(0, 0.05, 3) if off1 else None)
        for k in range(T):
            R = tR[k] @ rotvec(rng.normal(0, 2e-3, 3))
            if pinfo:
                A = rng_w.normal(size=(6, 6))
                W = A @ A.T + 6 * np.eye(6)
                wb.add_prior(i, k, tt[k], R, info=W * (3 / 4.592449e-06 / np.trace(W)))
            else:
                wb.add_prior(i, k, tt[k], R, IMU_INFO)
        for k in range(1, T if se3 else 0):
            p = k - 1 if se3 == "twist" else int(key[k])
            A = rng.normal(size=(6, 6))
            info = A @ A.T + 6 * np.eye(6)
            wb.add_se3(i, p, k, tR[p].T @ (tt[k] - tt[p]) + rng.normal(0, 0.01, 3), tR[p].T @ tR[k] @ rotvec(rng.normal(0, 0.01, 3)),
                       info * (6e4 / np.trace(info)), robust=bool(k % 5))
    return wb


def _tests_path():
    p = os.path.join(ROOT, "tests")
    if p not in sys.path:
        sys.path.insert(0, p)


def _arrow(la):
    _tests_path()
    import _arrow_cov_inputs as A
    return A.case_batch(la, "5_1"), A.SURVEYED


def _marginal(la):
    _tests_path()
    import _fixed_lag as F
    wb, drop = F.case_batch(la, "chain10")
    return wb, drop, F.ANCH


def _table_batch(la):
    _tests_path()
    import _edge_audit_cases as K
    import _general_cov_inputs as G
    return K._symmetric_table(G.chain_batch(la, 9650, 4, 8, True, nv_max=65, ragged=False), np.random.default_rng(9651)), G.ANCH


def _general(**kw):
    return lambda la: windows(la, 5100, 4, 8, se3="keys", **kw)


# name -> (what runs: "solve" / "covariance" / "marginal_prior" / "edge_chi2", batch builder, Jacobian modes, iterations, handle options, the kernel
# last_kernel_kind() must report — None where the entry reports none)
BOTH = ("analytic", "numeric")
CASES = {
    "general_lds": ("solve", _general(), BOTH, 3, GENERAL, "window_lm_kernel"),
    "general_lds_pinfo": ("solve", _general(pinfo=True), BOTH, 3, GENERAL, "window_lm_kernel"),
    "general_lds_off1": ("solve", _general(off1=True), BOTH, 3, GENERAL, "window_lm_kernel"),
    "general_hbm_one_word": ("solve", lambda la: windows(la, 5200, 2, 24, se3="keys"), BOTH, 3, GENERAL, "window_lm_kernel"),
    "general_eight_waves": ("solve", lambda la: windows(la, 5300, 2, 70, se3="keys"), ("numeric",), 3, GENERAL, "window_lm_kernel"),
    "general_skyline": ("solve", lambda la: windows(la, 5400, 1, 513, se3="keys"), ("analytic",), 2, GENERAL, "window_lm_kernel"),
    "chain_uwb_imu_12": ("solve", lambda la: windows(la, 6100, 64, 12), BOTH, 3, LANES, "chain_lm_kernel"),
    "chain_twist_15": ("solve", lambda la: windows(la, 6200, 64, 15, se3="twist"), BOTH, 3, LANES, "chain_lm_kernel"),
    "chain_uwb_imu_40": ("solve", lambda la: windows(la, 6300, 64, 40), BOTH, 3, LANES, "chain_lm_kernel"),
    "tree_lane_64": ("solve", lambda la: windows(la, 7100, 64, 16, se3="forest"), BOTH, 3, dict(LANES, tree=2), "tree_lm_kernel"),
    "tree_lane_2": ("solve", lambda la: windows(la, 7100, 2, 16, se3="forest"), BOTH, 3, dict(LANES, tree=2), "tree_lm_kernel"),
    "tree_wave_64": ("solve", lambda la: windows(la, 7100, 64, 16, se3="forest"), BOTH, 3, LANES, "tree_wave_kernel"),
    "tree_wave_2": ("solve", lambda la: windows(la, 7100, 2, 16, se3="forest"), BOTH, 3, LANES, "tree_wave_kernel"),
    "cov_chain6": ("covariance", lambda la: windows(la, 8100, 4, 12, all_anchors=True), BOTH, 3, {}, None),
    "cov_forest": ("covariance", lambda la: windows(la, 8200, 4, 16, se3="forest", all_anchors=True), BOTH, 3, LANES, None),
    "cov_envelope": ("covariance", lambda la: windows(la, 8300, 4, 8, se3="keys", all_anchors=True), BOTH, 3, {"covariance_general": 1}, None),
    "cov_envelope_table": ("covariance", lambda la: _table_batch(la), BOTH, 3, {"covariance_general": 1}, None),
    "cov_arrow": ("covariance", _arrow, BOTH, 3, {"arrow3": 1}, None),
    "marginal_prior": ("marginal_prior", _marginal, BOTH, 3, {}, None),
    "edge_audit": ("edge_chi2", _general(), ("analytic",), 3, {}, None),
}


def pack(a):
    """(key suffix, uint64 array): the array's own bits, or one digest per window when it is large"""
    a = np.ascontiguousarray(a)
    if a.nbytes > FULL_BYTES:
        rows = a.reshape(a.shape[0], -1)
        return "#rows", np.array([int.from_bytes(hashlib.sha256(r.tobytes()).digest()[:8], "little") for r in rows], dtype=np.uint64)
    if a.dtype == np.float64:
        return "", a.view(np.uint64)
    return "", a.astype(np.int64).view(np.uint64)


def run_case(la, name, jac):
    """{array name: uint64 array} of one case in one Jacobian mode, inputs ("in/..") and outputs ("out/.."), and the kernel the solve reports"""
    what, build, _, iters, options, _ = CASES[name]
    made = build(la)
    wb, extra = (made[0], made[1:]) if isinstance(made, tuple) else (made, ())
    anchors = extra[-1] if extra else ANCH
    rec = {"in/" + k: getattr(wb, k).copy() for k in wb.TABLES}
    for k in ("r_off1", "p_info"):
        if getattr(wb, k, None) is not None:
            rec["in/" + k] = getattr(wb, k).copy()
    s = la.WindowSolver(anchors, wb.B, *wb.caps, maximum_iteration=iters, jacobian=jac)
    for k, v in options.items():
        s.set_option(k, v)
    kind = None
    if what == "solve":
        rec["out/result"] = s.solve(wb).copy()
        rec["out/poses"] = wb.poses.copy()
        kind = s.last_kernel_kind()
    elif what == "covariance":
        rec["out/cov"], rec["out/mask"], rec["out/status"] = s.covariance(wb)
    elif what == "marginal_prior":
        for k, v in zip(("slot", "prior", "grad", "shift", "rank", "status"), s.marginal_prior(wb, extra[0])):
            rec["out/" + k] = v
    else:
        for k, v in zip(("r_chi2", "p_chi2", "s_chi2", "total", "active"), s.edge_chi2(wb)):
            rec["out/" + k] = v
    s.close()
    out = {}
    for k, v in rec.items():
        suffix, bits = pack(v)
        out[k + suffix] = bits
    return out, kind


def case_ids():
    return [(name, jac) for name, c in CASES.items() for jac in c[2]]


def main(argv):
    if len(argv) != 3:
        print(__doc__)
        return 1
    os.environ["LOCALIZATION_AMD_LIB"] = os.path.abspath(argv[1])
    sys.path.insert(0, ROOT)
    import localization_amd as la
    assert os.path.samefile(la.library_path(), argv[1]), la.library_path()
    out, left_out = {}, []
    for name, jac in case_ids():
        first, kind = run_case(la, name, jac)
        second, _ = run_case(la, name, jac)
        want = CASES[name][5]
        assert want is None or kind == want, (name, jac, kind, want)
        if first.keys() != second.keys() or any(not np.array_equal(first[k], second[k]) for k in first):
            left_out.append(f"{name}/{jac}: " + ", ".join(k for k in first if not np.array_equal(first[k], second.get(k))))
            continue
        print(f"{name}/{jac}: {kind or CASES[name][0]}, {sum(v.nbytes for v in first.values())} bytes")
        for k, v in first.items():
            out[f"{name}/{jac}/{k}"] = v
    np.savez_compressed(argv[2], **out)
    print(f"{argv[2]}: {len(out)} arrays, {os.path.getsize(argv[2])} bytes")
    for line in left_out:
        print("LEFT OUT (two runs differ): " + line)
    return 2 if left_out else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
