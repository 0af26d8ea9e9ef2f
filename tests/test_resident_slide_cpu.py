"""The resident fixed-lag slide (loc_window_slide_resident; DESIGN.md §2, "The resident slide") without a GPU:

* the numpy statement of the rule (tests/_slide_ref.slide_ref) applied to tests/_fixed_lag.first_window gives the GRAPH that
  tests/_fixed_lag.next_window builds — the oracle's chi2 at equal poses agrees to 1e-12 relative.  (A graph comparison, not a table
  comparison: next_window stores a smoothness edge (k - 1, k) as (k, k - 1) for odd SLOT k, so the stored orientation of every kept edge
  flips with the slot parity; the edge is the same.)  The slid batch passes the oracle's index checks: every row builds an edge;
* the integer half of the rule on the host (window_structure.cpp: slide_indices, with slide_rows_translation_only) through the stand-alone
  driver tests/host/slide_indices_driver.cpp, compiled with g++ under AddressSanitizer + UBSan and run as a program: held to slide_ref's
  integer tables on every case of tests/_slide_ref.CASES, and to every refusal."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _dense_prior_ref as D
import _fixed_lag as F
import _slide_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "localization_amd", "csrc")
I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31


def _marginals(wb, mode):
    refs = [D.marginal_ref(wb, i, F.ANCH, mode, 0) for i in range(wb.B)]
    return np.array([r["slot"] for r in refs], dtype=np.int32), np.stack([r["prior"] for r in refs])


def _chi2(wb, i):
    """the oracle's chi2 of window i at wb.poses, no iteration: the sum of e^T Omega e over the edges of the graph as built, e from the
    oracle's own error evaluation of every edge (which fails on an edge whose vertices it does not know: its index check)"""
    from oracle import oracle as O
    G, edges = D.graph(wb, i, F.ANCH)
    assert len(edges) == int(wb.counts[i, 1] + wb.counts[i, 2])
    total = 0.0
    for k, (_, info, _, _) in enumerate(edges):
        e = G.linearize(k, O.JAC_ANALYTIC)[0]
        total += float(e @ info @ e)
    return total


def test_slide_ref_builds_next_windows_graph():
    import localization_amd as la
    from oracle import oracle as O
    W = 6
    chains = [F.Chain(7900 + i, W + 3, 3 + i % 3) for i in range(8)]
    wb = F.first_window(la, chains, W)
    rng = np.random.default_rng(5)
    for step in range(1, 4):
        wb.poses[:, :, 9:] += rng.normal(0, 0.01, wb.poses[:, :, 9:].shape)   # any estimate: the rule moves rows, it does not solve
        slot, prior = _marginals(wb, O.JAC_ANALYTIC)
        pose, ranges = S.new_rows(chains, np.full(8, step + W - 1), np.full(8, W - 1))
        ref = S.slide_ref(la, wb, slot, prior, pose, ranges)
        nxt = F.next_window(la, wb, chains, step, W, slots=slot, rows=prior)
        assert np.array_equal(ref.counts, nxt.counts) and ref.poses.tobytes() == nxt.poses.tobytes()
        for i in range(8):
            nv, nr, npr, _ = (int(x) for x in ref.counts[i])
            assert (ref.r_idx[i, :nr, 0] >= 0).all() and (ref.r_idx[i, :nr] < nv).all() and (ref.r_idx[i, :nr, 1] >= -len(F.ANCH)).all()
            assert (ref.p_idx[i, :npr] >= 0).all() and (ref.p_idx[i, :npr] < nv).all()
            a, b = _chi2(ref, i), _chi2(nxt, i)
            print(f"slide {step} window {i}: chi2 {a:.15e} (rule) {b:.15e} (next_window)")
            assert a > 0 and abs(a - b) <= 1e-12 * abs(b), (step, i, a, b)
        wb = ref


# ---- the host's index function under AddressSanitizer + UBSan ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("slide_indices_driver")
    cxx = shutil.which("g++")
    assert cxx is not None, "g++ is needed to build tests/host/slide_indices_driver.cpp (the project's build() needs it as well)"
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    rocm = os.path.dirname(os.path.dirname(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")))
    src = [os.path.join(ROOT, "tests", "host", "slide_indices_driver.cpp"), os.path.join(CSRC, "window_structure.cpp")]
    logs = []
    for extra in (["-static-libasan", "-static-libubsan"], []):   # (the runtimes as archives where the compiler has them)
        r = subprocess.run([cxx, "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), "-I", CSRC, "-pthread", *flags, *extra, *src,
                            "-o", str(d / "driver")], capture_output=True, text=True)
        logs.append(" ".join(extra) + ": " + r.stderr[-1500:])
        if r.returncode == 0:
            return str(d / "driver")
    raise AssertionError("\n".join(logs))


def _poison(wb):
    """unused slots of the index tables hold values that fault or mislead whoever reads them"""
    for i in range(wb.B):
        _, nr, npr, _ = (int(x) for x in wb.counts[i])
        wb.r_idx[i, nr:] = (I32_MAX, I32_MIN)
        wb.p_idx[i, npr:] = I32_MIN
    return wb


def _write(f, wb, pose, ranges, priors, drop, n_anchors=len(F.ANCH), bw_max=None):
    """one batch in the driver's format, every table at exactly its capacity"""
    nv, nr, npr, _ = wb.caps
    rc, ri, rv = ranges if ranges is not None else (None, np.zeros((wb.B, 0, 2), dtype=np.int32), np.zeros((wb.B, 0, 5)))
    pc, pv = priors if priors is not None else (None, np.zeros((wb.B, 0, 18)))
    nrn, npn = ri.shape[1], pv.shape[1]
    np.array([nv, nr, npr, max(nv - 1, 0) if bw_max is None else bw_max, n_anchors, nrn, npn, drop is not None], dtype=np.int32).tofile(f)
    np.array([wb.B], dtype=np.int64).tofile(f)
    for a in (wb.counts, wb.r_idx[:, :nr], wb.p_idx[:, :npr]):
        np.ascontiguousarray(a, dtype=np.int32).tofile(f)
    for a in (drop, rc if nrn else None, ri, pc if npn else None):
        if a is not None:
            np.ascontiguousarray(a, dtype=np.int32).tofile(f)
    for a in (pose, rv, pv):
        np.ascontiguousarray(a, dtype=np.float64).tofile(f)


def _expected(ref):
    """the driver's lines for a slid batch"""
    lines = []
    mx = 0
    for i in range(ref.B):
        nv, nr, npr, _ = (int(x) for x in ref.counts[i])
        r = ref.r_idx[i, :nr].reshape(-1)
        mx = max([mx] + [-int(v) for v in ref.r_idx[i, :nr, 1] if v < 0])
        lines.append(f"{nv} {nr} {npr} :" + "".join(f" {int(v)}" for v in r) + " :" + "".join(f" {int(v)}" for v in ref.p_idx[i, :npr]))
    return [str(mx)] + lines


def _run(driver, path):
    r = subprocess.run([driver, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout.splitlines()


@pytest.mark.parametrize("name", list(S.CASES))
def test_host_index_rule(driver, tmp_path, name):
    import localization_amd as la
    from oracle import oracle as O
    wb, chains, spec = S.case_batch(la, name)
    path = tmp_path / "in.bin"
    expected = []
    with open(path, "wb") as f:
        for step in range(3):
            pose, ranges, priors, drop = S.next_inputs(wb, chains, spec)
            slot, prior = _marginals(wb, O.JAC_ANALYTIC)
            _write(f, _poison(wb), pose, ranges, priors, drop)
            wb = S.slide_ref(la, wb, slot, prior, pose, ranges, priors, drop)
            expected += ["0 1"] + _expected(wb)
    assert _run(driver, path) == expected


def test_host_refusals(driver, tmp_path):
    import localization_amd as la
    cases = []   # (batch, pose, ranges, priors, drop, kwargs, expected first line)

    def base(name="plain"):
        wb, chains, spec = S.case_batch(la, name)
        pose, ranges, priors, drop = S.next_inputs(wb, chains, spec)
        return _poison(wb), pose, (ranges[0].copy(), ranges[1].copy(), ranges[2].copy()), priors, drop

    def z_prior(count):
        pv = np.zeros((8, 1, 18)); pv[:, 0, 0] = pv[:, 0, 4] = pv[:, 0, 8] = 1.0; pv[:, 0, 12:] = S.Z_INFO
        return np.full(8, count, dtype=np.int32), pv

    wb, pose, ranges, priors, drop = base()
    wb.counts[5, 0] = 0
    cases.append((wb, pose, ranges, priors, drop, {}, "1 1"))                          # a window without poses
    for bad_count in (-1, F.NA_MAX + 3, I32_MAX, I32_MIN):
        wb, pose, ranges, priors, drop = base()
        ranges[0][3] = bad_count
        cases.append((wb, pose, ranges, priors, drop, {}, "2 1"))                      # a count outside [0, nr_new_max]
    wb, pose, ranges, priors, drop = base()
    cases.append((wb, pose, ranges, z_prior(2), drop, {}, "2 1"))                      # ... outside [0, np_new_max]
    for v0, v1 in ((3, 5), (5, 3), (6, 5), (5, 5), (-1, 5), (5, -1 - len(F.ANCH)), (5, I32_MIN), (I32_MAX, 4), (4, 4)):
        wb, pose, ranges, priors, drop = base()                                        # the new slot is 5: a range to slot nv - 3, a slot beyond, a self edge,
        ranges[1][6, int(ranges[0][6]) - 1] = (v0, v1)                                 # an anchor beyond the table, ... in the place of the link
        cases.append((wb, pose, ranges, priors, drop, {}, "3 1"))
    wb, pose, ranges, priors, drop = base()
    ranges[1][2, 0] = (4, -1)                                                          # a row on slot 4 alone is fine in front ...
    cases.append((wb, pose, ranges, priors, drop, {}, "0 1"))
    wb, pose, ranges, priors, drop = base()
    ranges[1][2, 1] = (4, -1)                                                          # ... and out of order after a row that names slot 5
    cases.append((wb, pose, ranges, priors, drop, {}, "3 1"))
    wb, pose, ranges, priors, drop = base()
    cases.append((wb, pose, ranges, priors, drop, dict(bw_max=0), "3 1"))              # a pose-to-pose row under bw_max = 0
    wb, chains, spec = S.case_batch(la, "plain")                                       # a full window that only grows (its rows name slot 6)
    grow = np.array([1, 1, 1, 0, 1, 1, 1, 1], dtype=np.int32)
    pose, ranges = S.new_rows(chains, spec["consumed"], 6 - grow)
    cases.append((_poison(wb), pose, ranges, None, grow, {}, "4 1"))
    wb, chains, spec = S.case_batch(la, "plain")                                       # a doubled link in the fullest window: nr_max + 1
    full = int(np.argmax(wb.counts[:, 1]))
    pose, ranges = S.new_rows(chains, spec["consumed"], np.full(8, 5), doubled=(full,))
    small = la.WindowBatch(8, wb.caps[0], int(wb.counts[full, 1]), wb.caps[2], 0)
    small.counts[:] = wb.counts; small.r_idx[:] = wb.r_idx[:, :small.caps[1]]; small.p_idx[:] = wb.p_idx
    cases.append((_poison(small), pose, ranges, None, None, {}, "5 1"))
    wb, pose, ranges, priors, drop = base("long")                                      # three kept priors + the carried one + a new one: np_max + 1
    cases.append((wb, pose, ranges, z_prior(1), drop, {}, "6 1"))
    # the value half: a rotated new pose, a lever arm on a new range, rotation information on a new prior
    wb, pose, ranges, priors, drop = base()
    pose = pose.copy(); pose[4, :9] = np.array([0, -1, 0, 1, 0, 0, 0, 0, 1.0])
    cases.append((wb, pose, ranges, priors, drop, {}, "0 0"))
    wb, pose, ranges, priors, drop = base()
    ranges[2][1, 0, 3] = 1e-300
    cases.append((wb, pose, ranges, priors, drop, {}, "0 0"))
    wb, pose, ranges, priors, drop = base()
    pc, pv = z_prior(0); pc[7] = 1; pv[7, 0, 16] = 1e-300
    cases.append((wb, pose, ranges, (pc, pv), drop, {}, "0 0"))
    for k, (wb, pose, ranges, priors, drop, kw, want) in enumerate(cases):
        path = tmp_path / f"case{k}.bin"
        with open(path, "wb") as f:
            _write(f, wb, pose, ranges, priors, drop, **kw)
        assert _run(driver, path)[0] == want, (k, want)

