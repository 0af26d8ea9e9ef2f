"""The per-window admission rule of loc_window_slide_resident_dev (localization_amd/csrc/slide_admit.h; DESIGN.md §2, "The resident slide")
without a GPU.  The shared function is what the device prologue restates, so it is held here, window by window, to

* the batch-wide rule of loc_window_slide_resident asked about one window alone: slide_indices(apply = false)'s first `bad`, and code 7 where
  that is 0 and slide_rows_translation_only says no — through the stand-alone driver tests/host/slide_admit_driver.cpp, compiled with g++
  under AddressSanitizer + UBSan and run as a program (every window's tables handed over at exactly the size its counts name);
* a numpy statement of the rule written below (_admit_np).

Cases: the next inputs of every case of tests/_slide_ref.CASES (all admitted), every refusal tests/test_gpu_resident_slide_dev.py puts on the
GPU (tests/_slide_dev_cases.py), and 480 random windows whose counts and indices are drawn around every bound (fixed seed)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _fixed_lag as F
import _slide_dev_cases as K
import _slide_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "localization_amd", "csrc")
I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31
ONE_BITS = np.float64(1.0).view(np.uint64)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("slide_admit_driver")
    cxx = shutil.which("g++")
    assert cxx is not None, "g++ is needed to build tests/host/slide_admit_driver.cpp (the project's build() needs it as well)"
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    rocm = os.path.dirname(os.path.dirname(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")))
    src = [os.path.join(ROOT, "tests", "host", "slide_admit_driver.cpp"), os.path.join(CSRC, "window_structure.cpp")]
    logs = []
    for extra in (["-static-libasan", "-static-libubsan"], []):   # (the runtimes as archives where the compiler has them)
        r = subprocess.run([cxx, "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), "-I", CSRC, "-pthread", *flags, *extra, *src,
                            "-o", str(d / "driver")], capture_output=True, text=True)
        logs.append(" ".join(extra) + ": " + r.stderr[-1500:])
        if r.returncode == 0:
            return str(d / "driver")
    raise AssertionError("\n".join(logs))


class Batch:
    """one batch in the driver's format: plain arrays, every table at exactly its capacity"""

    def __init__(self, caps, bw_max, n_anchors, counts, r_idx, p_idx, drop, pose, ranges, priors):
        self.nv_max, self.nr_max, self.np_max = (int(x) for x in caps[:3])
        self.bw_max, self.n_anchors = int(bw_max), int(n_anchors)
        self.counts = np.ascontiguousarray(counts, dtype=np.int32)
        self.B = len(self.counts)
        self.r_idx = np.ascontiguousarray(r_idx, dtype=np.int32).reshape(self.B, self.nr_max, 2)
        self.p_idx = np.ascontiguousarray(p_idx, dtype=np.int32).reshape(self.B, self.np_max)
        self.drop = None if drop is None else np.ascontiguousarray(np.broadcast_to(drop, (self.B,)), dtype=np.int32)
        self.pose = np.ascontiguousarray(pose, dtype=np.float64).reshape(self.B, 12)
        rc, ri, rv = ranges if ranges is not None else (None, np.zeros((self.B, 0, 2), dtype=np.int32), np.zeros((self.B, 0, 5)))
        pc, pv = priors if priors is not None else (None, np.zeros((self.B, 0, 18)))
        self.ri, self.rv, self.pv = np.ascontiguousarray(ri, dtype=np.int32), np.ascontiguousarray(rv, dtype=np.float64), np.ascontiguousarray(pv, dtype=np.float64)
        self.nrn, self.npn = self.ri.shape[1], self.pv.shape[1]
        self.rc = np.zeros(self.B, dtype=np.int32) if not self.nrn else np.ascontiguousarray(rc, dtype=np.int32)
        self.pc = np.zeros(self.B, dtype=np.int32) if not self.npn else np.ascontiguousarray(pc, dtype=np.int32)

    def write(self, f):
        np.array([self.nv_max, self.nr_max, self.np_max, self.bw_max, self.n_anchors, self.nrn, self.npn, self.drop is not None], dtype=np.int32).tofile(f)
        np.array([self.B], dtype=np.int64).tofile(f)
        for a in (self.counts, self.r_idx, self.p_idx, self.drop, self.rc if self.nrn else None, self.ri, self.pc if self.npn else None, self.pose, self.rv, self.pv):
            if a is not None:
                a.tofile(f)


def _poisoned(wb):
    """a WindowBatch's index tables with values in the unused slots that mislead whoever reads them"""
    r_idx, p_idx = wb.r_idx.copy(), wb.p_idx.copy()
    for i in range(wb.B):
        _, nr, npr, _ = (int(x) for x in wb.counts[i])
        r_idx[i, nr:] = (I32_MAX, I32_MIN)
        p_idx[i, npr:] = I32_MIN
    return r_idx, p_idx


def _of_window_batch(wb, pose, ranges, priors, drop, bw_max=None):
    r_idx, p_idx = _poisoned(wb)
    return Batch(wb.caps, max(wb.caps[0] - 1, 0) if bw_max is None else bw_max, len(F.ANCH), wb.counts, r_idx[:, :wb.caps[1]], p_idx[:, :wb.caps[2]],
                 drop, pose, ranges, priors)


def _identity_bits(v):
    want = np.zeros(9, dtype=np.uint64); want[[0, 4, 8]] = ONE_BITS
    return bool((np.ascontiguousarray(v[:9], dtype=np.float64).view(np.uint64) == want).all())


def _admit_np(b, i):
    """the rule of DESIGN.md §2 for window i of Batch b: the code of the first check that fails, 0 if none does"""
    nv, nr, npr, _ = (int(x) for x in b.counts[i])
    drop = True if b.drop is None else bool(b.drop[i])
    nrn, npn = int(b.rc[i]), int(b.pc[i])
    if nv <= 0:
        return 1
    if not (0 <= nrn <= b.nrn and 0 <= npn <= b.npn):
        return 2
    s = nv - int(drop)
    rows = b.ri[i, :nrn].astype(np.int64)
    v0, v1 = rows[:, 0], rows[:, 1]
    ok0 = (v0 == s) | ((v0 == s - 1) & (v0 >= 0))
    ok1 = np.where(v1 < 0, v1 >= -b.n_anchors, ((v1 == s) | (v1 == s - 1)) & (v1 != v0) & (b.bw_max >= 1))
    names = (v0 == s) | (v1 == s)
    named_before = np.concatenate([[False], np.logical_or.accumulate(names)[:-1]]) if nrn else names
    if (~ok0 | ~ok1 | (named_before & ~names)).any():
        return 3
    old = b.r_idx[i, :nr].astype(np.int64)
    on0 = (old[:, 0] == 0) | (old[:, 1] == 0)
    r_kept = int((~on0).sum()) if drop else nr
    carried = int(drop and bool((on0 & (old[:, 1] >= 0)).any()))
    p_kept = int((b.p_idx[i, :npr] != 0).sum()) if drop else npr
    if s + 1 > b.nv_max:
        return 4
    if r_kept + nrn > b.nr_max:
        return 5
    if carried + p_kept + npn > b.np_max:
        return 6
    lever = b.rv[i, :nrn, 2:5]
    pv = b.pv[i, :npn]
    if not _identity_bits(b.pose[i]) or (lever != 0.0).any() or (pv[:, 15:18] != 0.0).any() or not all(_identity_bits(p) for p in pv):
        return 7
    return 0


def _check(driver, tmp_path, batches, name):
    """the driver's three figures for every window of the batches against each other and against the numpy rule; returns the codes"""
    path = tmp_path / f"{name}.bin"
    with open(path, "wb") as f:
        for b in batches:
            b.write(f)
    r = subprocess.run([driver, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    got = np.array([[int(x) for x in line.split()] for line in r.stdout.splitlines()], dtype=int)
    want = np.array([_admit_np(b, i) for b in batches for i in range(b.B)], dtype=int)
    assert got.shape == (len(want), 3), (got.shape, len(want))
    code, bad, translation = got.T
    host_rule = np.where(bad != 0, bad, np.where(translation == 1, 0, 7))
    where = np.flatnonzero((code != host_rule) | (code != want))
    assert where.size == 0, (name, where[:10], code[where[:10]], host_rule[where[:10]], want[where[:10]])
    return code


@pytest.mark.parametrize("name", list(S.CASES))
def test_cases_next_inputs_are_admitted(driver, tmp_path, name):
    import localization_amd as la
    from oracle import oracle as O
    import _dense_prior_ref as D
    wb, chains, spec = S.case_batch(la, name)
    batches = []
    for step in range(3):
        pose, ranges, priors, drop = S.next_inputs(wb, chains, spec)
        batches.append(_of_window_batch(wb, pose, ranges, priors, drop))
        refs = [D.marginal_ref(wb, i, F.ANCH, O.JAC_ANALYTIC, 0) for i in range(wb.B)]
        slot, prior = np.array([r["slot"] for r in refs], dtype=np.int32), np.stack([r["prior"] for r in refs])
        wb = S.slide_ref(la, wb, slot, prior, pose, ranges, priors, drop)
    assert not _check(driver, tmp_path, batches, name).any()


@pytest.mark.parametrize("variant", list(K.CODES))
def test_the_gpu_tests_refusals(driver, tmp_path, variant):
    import localization_amd as la
    wb, chains, spec = K.tight_batch(la)
    if variant == "c":
        K.empty_window(wb, 1)
    pose, ranges, priors, drop = K.refusing_inputs(wb, chains, spec, variant)
    code = _check(driver, tmp_path, [_of_window_batch(wb, pose, ranges, priors, drop)], variant)
    assert code.tolist() == K.CODES[variant]
    wb, chains, spec = K.tight_batch(la)
    assert not _check(driver, tmp_path, [_of_window_batch(wb, *K.benign_inputs(wb, chains, spec))], variant + "_benign").any()


def _random_batch(rng, B=32):
    """B windows of ordered translation-only chains under random tight capacities; counts and indices of the new rows around every bound"""
    nv_max = int(rng.integers(1, 7))
    na = int(rng.integers(1, 4))
    n_anchors = int(rng.integers(1, 5))
    bw_max = int(rng.integers(0, 2)) if nv_max > 1 else 0
    nrn, npn = int(rng.integers(0, 7)), int(rng.integers(0, 3))
    nr_max = nv_max * na + (nv_max - 1) * bw_max + int(rng.integers(0, 3))
    np_max = int(rng.integers(0, 4))
    counts = np.zeros((B, 4), dtype=np.int32)
    r_idx = np.full((B, nr_max, 2), I32_MIN, dtype=np.int32)
    p_idx = np.full((B, np_max), I32_MIN, dtype=np.int32)
    for i in range(B):
        nv = 0 if rng.random() < 0.08 else nv_max if rng.random() < 0.5 else int(rng.integers(1, nv_max + 1))   # (full windows: the capacities bind)
        rows, priors = [], []
        for v in range(nv):
            if v and bw_max and rng.random() < 0.8:
                rows.append((v, v - 1) if rng.random() < 0.5 else (v - 1, v))
            rows += [(v, -1 - int(rng.integers(n_anchors))) for _ in range(na if rng.random() < 0.7 else int(rng.integers(0, na + 1)))]
            if len(priors) < np_max and rng.random() < 0.4:
                priors.append(v)
        counts[i, :3] = (nv, len(rows), len(priors))
        r_idx[i, :len(rows)] = np.array(rows, dtype=np.int32).reshape(-1, 2)
        p_idx[i, :len(priors)] = priors
    drop = None if rng.random() < 0.25 else rng.integers(0, 2, B).astype(np.int32)
    s = counts[:, 0] - (1 if drop is None else (drop != 0).astype(int))   # the new slot of every window
    rc = rng.choice([-1, 0, 1, max(nrn - 1, 0), nrn, nrn + 1, I32_MAX, I32_MIN], B, p=[.05, .1, .15, .2, .4, .06, .02, .02]).astype(np.int32)
    pc = rng.choice([-1, 0, npn, npn + 1], B, p=[.03, .45, .45, .07]).astype(np.int32)
    ri = np.zeros((B, nrn, 2), dtype=np.int32)
    for i in range(B):
        for e in range(nrn):
            if rng.random() < 0.85:   # a row the rule takes: on s or s - 1, to an anchor or the other of the two
                v0 = int(s[i]) - int(rng.random() < (0.5 if e == 0 else 0.1))
                v1 = -1 - int(rng.integers(n_anchors)) if rng.random() < 0.7 else 2 * int(s[i]) - 1 - v0
            else:
                v0 = int(s[i]) + int(rng.choice([-2, -1, 0, 1]))
                v1 = int(rng.choice([int(s[i]) - 2, int(s[i]) - 1, int(s[i]), int(s[i]) + 1, -1, -n_anchors, -n_anchors - 1, I32_MIN, I32_MAX]))
            ri[i, e] = (v0, v1)
    pose = np.zeros((B, 12)); pose[:, [0, 4, 8]] = 1.0; pose[:, 9:] = rng.normal(size=(B, 3))
    rv = np.zeros((B, nrn, 5)); rv[:, :, 0] = rng.uniform(1, 5, (B, nrn)); rv[:, :, 1] = F.RANGE_INFO
    pv = np.zeros((B, npn, 18)); pv[:, :, [0, 4, 8]] = 1.0; pv[:, :, 9:15] = rng.normal(size=(B, npn, 6))
    for i in np.flatnonzero(rng.random(B) < 0.2):   # one value that is not translation-only (or only looks like it: -0.0 in a rotation, 0.0 * -1 in a lever arm)
        kind = int(rng.integers(6))
        if kind == 0: pose[i, int(rng.integers(9))] = rng.choice([-0.0, 0.5, np.nan])
        elif kind == 1 and nrn: rv[i, int(rng.integers(nrn)), 2 + int(rng.integers(3))] = rng.choice([1e-300, -0.0, np.nan])
        elif kind == 2 and npn: pv[i, int(rng.integers(npn)), int(rng.integers(9))] = rng.choice([-0.0, 1e-300])
        elif kind == 3 and npn: pv[i, int(rng.integers(npn)), 15 + int(rng.integers(3))] = rng.choice([1e-300, -0.0, np.inf])
        elif kind == 4: pose[i, 0] = np.nextafter(1.0, 2.0)
    return Batch((nv_max, nr_max, np_max), bw_max, n_anchors, counts, r_idx, p_idx, drop, pose, (rc, ri, rv), (pc, pv))


def test_random_windows_around_every_bound(driver, tmp_path):
    rng = np.random.default_rng(20240607)
    code = _check(driver, tmp_path, [_random_batch(rng) for _ in range(15)], "random")
    seen = np.bincount(code, minlength=8)
    print("windows per code 0 .. 7:", seen.tolist())
    assert (seen > 0).all(), seen
