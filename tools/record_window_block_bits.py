#!/usr/bin/env python3
"""Bit records of window_lm_kernel on every structure its factorisations tell apart (localization_amd/csrc/window_block_device.h).

    tools/record_window_block_bits.py LIBRARY.so OUT.npz

runs the cases below on LIBRARY (any build of liblocalization_amd.so: the golden file tests/golden/window_block_steps_parent_bits.npz was
recorded with the library of commit 4fd0441, the parent of the commit that added this tool: the kernel that every attempt to turn a
written-out block step of factor_and_solve_sparse / factor_and_solve_small into a call of that header has to reproduce) and writes one 64-bit digest per window — the first 8 bytes of the sha256 over the window's solved poses and its result row — as uint64.
Every case runs twice; a case whose two runs differ is left out and named on stdout (exit status 2).
tests/test_gpu_window_block_bits.py runs the same cases on the built library and requires every digest to be equal.

Cases: every batch of tests/_graph_families.py in the Jacobian modes its suite runs, as built, relabelled and (NATURAL batches) in the caller's
order, each pinned to window_lm_kernel; the same again with a full information matrix on every prior (the batches that carry priors: the
6-DoF ones); and the failed factorisations — "third negated" (every third range's information negated in every window) on lds6, ws6 and wide6,
"root" (the unknown anchors' position priors of selfcal6 at -1e9): numeric refusals after steps were taken, the only inputs on which the pivot
rule of a Cholesky site decides anything.
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

VARIANTS = ("as built", "relabelled", "caller's order")
THIRD_NEGATED = ("lds6", "ws6", "wide6")


def _families():
    import _graph_families as F
    return F


def case_ids():
    """(group, batch, Jacobian mode, variant)"""
    F = _families()
    out = []
    for group in ("plain", "full information"):
        for name, spec in F.BATCHES.items():
            if group == "full information" and not spec[0]:      # (a 3-DoF batch carries no prior)
                continue
            for mode in F.batch_modes(name):
                out += [(group, name, mode, v) for v in VARIANTS if v != "caller's order" or name in F.NATURAL]
    out += [("third negated", name, mode, "as built") for name in THIRD_NEGATED for mode in F.MODES]
    out.append(("root", "selfcal6", "analytic", "as built"))
    return out


def full_information(wb, seed):
    """every prior's diagonal information replaced by a full symmetric positive definite 6x6 of the same trace (p_val keeps its diagonal)"""
    rng = np.random.default_rng(seed)
    wb.p_info = np.zeros((wb.B, max(wb.caps[2], 1), 36))
    for i in range(wb.B):
        for e in range(int(wb.counts[i, 2])):
            A = rng.normal(size=(6, 6))
            W = A @ A.T + 6 * np.eye(6)
            W *= wb.p_val[i, e, 12:].sum() / np.trace(W)
            wb.p_info[i, e] = W.reshape(36)
            wb.p_val[i, e, 12:] = np.diag(W)
    return wb


def build_case(group, name, variant):
    F = _families()
    wb = F.relabelled_batch(name) if variant == "relabelled" else F.build_batch(name)
    if group == "full information":
        full_information(wb, F.BATCHES[name][2] + 5)
    elif group == "third negated":
        for i in range(wb.B):
            wb.r_val[i, :int(wb.counts[i, 1]):3, 1] *= -1.0
    elif group == "root":
        for i in range(wb.B):
            n = int(wb.counts[i, 2])
            anchors = (wb.p_val[i, :n, 12] == 1.0) & (wb.p_val[i, :n, 15] == 0.0)      # position priors: the unknown anchors'
            assert anchors.any()
            wb.p_val[i, :n, 12:15][anchors] = -1e9
    return wb


def run_case(la, group, name, mode, variant):
    """(uint64 digest per window, result rows, the kernel the solve reports)"""
    from _general_cov_inputs import ANCH
    F = _families()
    caps = F.batch_caps(name)
    wb = build_case(group, name, variant)
    s = la.WindowSolver(ANCH, wb.B, *caps[:4], maximum_iteration=10, bw_max=caps[4], jacobian=mode, natural_order=variant == "caller's order",
                        chain_threshold=0)
    for opt in ("arrow3", "tree", "wave3", "wave6", "chain3"):
        s.set_option(opt, 0)
    res = s.solve(wb).copy()
    kind = s.last_kernel_kind()
    s.close()
    digest = [int.from_bytes(hashlib.sha256(wb.poses[i].view(np.uint64).tobytes() + res[i].view(np.uint64).tobytes()).digest()[:8], "little")
              for i in range(wb.B)]
    return np.array(digest, dtype=np.uint64), res, kind


def key(case):
    return "/".join(case)


def main(argv):
    if len(argv) != 3:
        print(__doc__)
        return 1
    os.environ["LOCALIZATION_AMD_LIB"] = os.path.abspath(argv[1])
    import localization_amd as la
    assert os.path.samefile(la.library_path(), argv[1]), la.library_path()
    out, left_out = {}, []
    for case in case_ids():
        first, res, kind = run_case(la, *case)
        second, _, _ = run_case(la, *case)
        assert kind == "window_lm_kernel", (case, kind)
        if not np.array_equal(first, second):
            left_out.append(key(case))
            continue
        print(f"{key(case)}: outer {res[:, 3].astype(int).tolist()} trials {res[:, 4].astype(int).tolist()} terminated {res[:, 5].astype(int).tolist()}")
        out[key(case)] = first
    np.savez_compressed(argv[2], **out)
    print(f"{argv[2]}: {len(out)} cases, {os.path.getsize(argv[2])} bytes")
    for line in left_out:
        print("LEFT OUT (two runs differ): " + line)
    return 2 if left_out else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
