"""The per-window admission rule of loc_window_slide_plain_resident_dev (localization_amd/csrc/slide_plain_admit.h; DESIGN.md §2, "The plain drop
for 6-DoF chain windows") without a GPU.  The shared function is what the device prologue of window_slide_plain_kernel.hip restates, so it is
held here, window by window, to a numpy statement of the rule (_admit_np) — through the stand-alone driver
tests/host/slide_plain_admit_driver.cpp, compiled with g++ under AddressSanitizer + UBSan and run as a program.  Every window's tables are
handed over at exactly the size its counts name, and the unused slots of the file are poisoned with INT32_MIN / INT32_MAX.

Cases: the next inputs of every case of tests/_slide_plain_ref.CASES (all admitted), every refusal tests/test_gpu_resident_slide_plain.py puts
on the GPU (and that its inputs are admitted in every other window), and 480 random windows per verdict whose counts and indices are drawn
around every bound (fixed seed)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _slide_plain_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "localization_amd", "csrc")
I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31
PAIR_RULE = {"chain": 0, "wave6": 1, "wave6s": 2}
CASE_RULE = {"imu": "wave6", "lidar": "wave6", "ragged": "wave6", "twist": "wave6s", "long": "chain"}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("slide_plain_admit_driver")
    cxx = shutil.which("g++")
    assert cxx is not None, "g++ is needed to build tests/host/slide_plain_admit_driver.cpp (the project's build() needs it as well)"
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    src = [os.path.join(ROOT, "tests", "host", "slide_plain_admit_driver.cpp")]
    logs = []
    for extra in (["-static-libasan", "-static-libubsan"], []):   # (the runtimes as archives where the compiler has them)
        r = subprocess.run([cxx, "-std=c++17", "-I", CSRC, *flags, *extra, *src, "-o", str(d / "driver")], capture_output=True, text=True)
        logs.append(" ".join(extra) + ": " + r.stderr[-1500:])
        if r.returncode == 0:
            return str(d / "driver")
    raise AssertionError("\n".join(logs))


class Batch:
    """one batch in the driver's format: plain arrays, every table at exactly its capacity"""

    def __init__(self, caps, bw_max, n_anchors, rule, counts, r_idx, p_idx, s_idx, drop, ranges, priors, se3):
        self.nv_max, self.nr_max, self.np_max, self.ns_max = (int(x) for x in caps)
        self.bw_max, self.n_anchors, self.rule = int(bw_max), int(n_anchors), PAIR_RULE[rule]
        self.counts = np.ascontiguousarray(counts, dtype=np.int32)
        self.B = len(self.counts)
        self.r_idx = np.ascontiguousarray(r_idx, dtype=np.int32).reshape(self.B, self.nr_max, 2)
        self.p_idx = np.ascontiguousarray(p_idx, dtype=np.int32).reshape(self.B, self.np_max)
        self.s_idx = np.ascontiguousarray(s_idx, dtype=np.int32).reshape(self.B, self.ns_max, 4)
        self.drop = None if drop is None else np.ascontiguousarray(np.broadcast_to(drop, (self.B,)), dtype=np.int32)
        self.rc, self.ri = np.ascontiguousarray(ranges[0], dtype=np.int32), np.ascontiguousarray(ranges[1], dtype=np.int32)
        self.pc, self.npn = np.ascontiguousarray(priors[0], dtype=np.int32), int(priors[1])
        self.sc, self.si = np.ascontiguousarray(se3[0], dtype=np.int32), np.ascontiguousarray(se3[1], dtype=np.int32)
        self.nrn, self.nsn = self.ri.shape[1], self.si.shape[1]

    def write(self, f):
        np.array([self.nv_max, self.nr_max, self.np_max, self.ns_max, self.bw_max, self.n_anchors, self.rule, self.nrn, self.npn, self.nsn,
                  self.drop is not None, 0], dtype=np.int32).tofile(f)
        np.array([self.B], dtype=np.int64).tofile(f)
        for a in (self.counts, self.r_idx, self.p_idx, self.s_idx, self.drop, self.rc, self.pc, self.sc, self.ri, self.si):
            if a is not None:
                a.tofile(f)


def _of_window_batch(wb, rule, inputs):
    """a WindowBatch and a slide's inputs as a Batch; the unused slots of the index tables hold values that mislead whoever reads them"""
    pose, (rc, ri, _), (pc, pv), (sc, si, _), drop = inputs
    nv_max, nr_max, np_max, ns_max = wb.caps
    r_idx, p_idx, s_idx = wb.r_idx[:, :nr_max].copy(), wb.p_idx[:, :np_max].copy(), wb.s_idx[:, :ns_max].copy()
    ri, si = np.array(ri, dtype=np.int32), np.array(si, dtype=np.int32)
    for i in range(wb.B):
        _, nr, npr, ns = (int(x) for x in wb.counts[i])
        r_idx[i, nr:] = (I32_MAX, I32_MIN); p_idx[i, npr:] = I32_MIN; s_idx[i, ns:] = (I32_MIN, I32_MAX, I32_MIN, I32_MAX)
        if 0 <= rc[i] <= ri.shape[1]: ri[i, int(rc[i]):] = (I32_MIN, I32_MAX)
        if 0 <= sc[i] <= si.shape[1]: si[i, int(sc[i]):] = (I32_MAX, I32_MIN, I32_MAX, I32_MIN)
    return Batch(wb.caps, max(nv_max - 1, 0), len(P.ANCH), rule, wb.counts, r_idx, p_idx, s_idx, drop, (rc, ri), (pc, pv.shape[1]), (sc, si))


def _admit_np(b, i):
    """the rule of DESIGN.md §2 for window i of Batch b: the code of the first check that fails, 0 if none does"""
    nv, nr, npr, ns = (int(x) for x in b.counts[i])
    drop = True if b.drop is None else bool(b.drop[i])
    nrn, npn, nsn = (int(b.rc[i]) if b.nrn else 0), (int(b.pc[i]) if b.npn else 0), (int(b.sc[i]) if b.nsn else 0)
    if nv <= 0:
        return 1
    if not (0 <= nrn <= b.nrn and 0 <= npn <= b.npn and 0 <= nsn <= b.nsn):
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
    pair = b.si[i, :nsn, :2].astype(np.int64)
    if nsn and not (s >= 1 and b.bw_max >= 1 and all(sorted(p) == [s - 1, s] for p in pair.tolist())):
        return 3
    old_r, old_p, old_s = b.r_idx[i, :nr], b.p_idx[i, :npr], b.s_idx[i, :ns, :2]
    r_kept = int(((old_r != 0).all(axis=1)).sum()) if drop else nr
    p_kept = int((old_p != 0).sum()) if drop else npr
    s_kept = int(((old_s != 0).all(axis=1)).sum()) if drop else ns
    for code, total, cap in ((4, s + 1, b.nv_max), (5, r_kept + nrn, b.nr_max), (6, p_kept + npn, b.np_max), (8, s_kept + nsn, b.ns_max)):
        if total > cap:
            return code
    pairs = int((v1 >= 0).sum())
    if (b.rule == 1 and (nsn > 0 or pairs > 1)) or (b.rule == 2 and (nsn > 1 or pairs > 1)):
        return 9
    return 0


def _check(driver, tmp_path, batches, name):
    """the driver's code for every window of the batches against the numpy rule; returns the codes"""
    path = tmp_path / f"{name}.bin"
    with open(path, "wb") as f:
        for b in batches:
            b.write(f)
    r = subprocess.run([driver, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    code = np.array([int(line) for line in r.stdout.split()], dtype=int)
    want = np.array([_admit_np(b, i) for b in batches for i in range(b.B)], dtype=int)
    assert code.shape == want.shape, (code.shape, want.shape)
    where = np.flatnonzero(code != want)
    assert where.size == 0, (name, where[:10], code[where[:10]], want[where[:10]])
    return code


@pytest.mark.parametrize("name", list(P.CASES))
def test_cases_next_inputs_are_admitted(driver, tmp_path, name):
    import localization_amd as la
    wb, streams, spec = P.case_batch(la, name)
    batches = []
    for _ in range(P.SLIDES):
        inputs = P.next_inputs(wb, streams, spec)
        batches.append(_of_window_batch(wb, CASE_RULE[name], inputs))
        wb = P.slide_plain_ref(la, wb, *inputs)
    assert not _check(driver, tmp_path, batches, name).any()


@pytest.mark.parametrize("variant", list(P.REFUSALS))
def test_the_gpu_tests_refusals(driver, tmp_path, variant):
    import localization_amd as la
    case, want = P.REFUSALS[variant]
    wb, streams, spec = P.refusal_batch(la, variant)
    benign, refusing = P.refusing_inputs(wb, streams, spec, variant)
    codes = [0] * 8
    codes[P.REFUSED] = want
    assert _check(driver, tmp_path, [_of_window_batch(wb, CASE_RULE[case], refusing)], variant).tolist() == codes
    codes[P.REFUSED] = 1 if variant == "no_poses" else 0   # the same inputs without the broken rule: every window slides
    assert _check(driver, tmp_path, [_of_window_batch(wb, CASE_RULE[case], benign)], variant + "_benign").tolist() == codes


def _random_batch(rng, rule, B=32):
    """B windows of ordered 6-DoF chains under random tight capacities; counts and indices of the new rows around every bound"""
    nv_max = int(rng.integers(1, 7))
    na = int(rng.integers(1, 3))
    n_anchors = int(rng.integers(1, 5))
    bw_max = int(rng.random() < 0.85) if nv_max > 1 else 0
    se3 = 0 if rule == "wave6" else int(rng.integers(1, 3)) if rule == "chain" else 1
    nrn, npn, nsn = int(rng.integers(0, 5)), int(rng.integers(0, 3)), int(rng.integers(0, 3))
    nr_max = nv_max * na + (nv_max - 1) * bw_max + int(rng.integers(0, 2))
    np_max = nv_max + int(rng.integers(0, 2))
    ns_max = (nv_max - 1) * bw_max * se3 + int(rng.integers(0, 2))
    counts = np.zeros((B, 4), dtype=np.int32)
    r_idx = np.full((B, nr_max, 2), I32_MIN, dtype=np.int32)
    p_idx = np.full((B, np_max), I32_MIN, dtype=np.int32)
    s_idx = np.full((B, ns_max, 4), I32_MAX, dtype=np.int32)
    for i in range(B):
        nv = 0 if rng.random() < 0.06 else nv_max if rng.random() < 0.6 else int(rng.integers(1, nv_max + 1))   # (full windows: the capacities bind)
        rows, priors, twists = [], [], []
        for v in range(nv):
            if v and bw_max and rng.random() < 0.9:
                rows.append((v, v - 1) if rng.random() < 0.5 else (v - 1, v))
            rows += [(v, -1 - int(rng.integers(n_anchors))) for _ in range(na if rng.random() < 0.8 else int(rng.integers(0, na + 1)))]
            if rng.random() < 0.9:
                priors.append(v)
            if v and bw_max:
                twists += [((v, v - 1) if rng.random() < 0.5 else (v - 1, v)) + (int(rng.integers(2)), 0) for _ in range(se3 if rng.random() < 0.9 else 0)]
        counts[i] = (nv, len(rows), len(priors), len(twists))
        r_idx[i, :len(rows)] = np.array(rows, dtype=np.int32).reshape(-1, 2)
        p_idx[i, :len(priors)] = priors
        s_idx[i, :len(twists)] = np.array(twists, dtype=np.int32).reshape(-1, 4)
    drop = None if rng.random() < 0.25 else (rng.random(B) < 0.75).astype(np.int32)
    s = counts[:, 0] - (1 if drop is None else (drop != 0).astype(int))   # the new slot of every window
    rc = rng.choice([-1, 0, 1, max(nrn - 1, 0), nrn, nrn + 1, I32_MAX, I32_MIN], B, p=[.02, .1, .2, .3, .33, .03, .01, .01]).astype(np.int32)
    pc = rng.choice([-1, 0, 1, npn, npn + 1], B, p=[.02, .2, .5, .25, .03]).astype(np.int32)
    sc = rng.choice([-1, 0, 1, nsn, nsn + 1], B, p=[.02, .5 if rule == "wave6" else .2, .2 if rule == "wave6" else .5, .25, .03]).astype(np.int32)
    ri = np.zeros((B, nrn, 2), dtype=np.int32)
    si = np.zeros((B, nsn, 4), dtype=np.int32)
    for i in range(B):
        paired = False
        for e in range(nrn):
            if rng.random() < 0.97:   # a row the rule takes: on s or s - 1, to an anchor or (mostly once) the other of the two
                v0 = int(s[i]) - int(rng.random() < (0.3 if e == 0 else 0.03))
                to_pose = rng.random() < (0.06 if paired else 0.4)
                v1 = 2 * int(s[i]) - 1 - v0 if to_pose else -1 - int(rng.integers(n_anchors))
                paired = paired or to_pose
            else:
                v0 = int(s[i]) + int(rng.choice([-2, -1, 0, 1]))
                v1 = int(rng.choice([int(s[i]) - 2, int(s[i]) - 1, int(s[i]), int(s[i]) + 1, -1, -n_anchors, -n_anchors - 1, I32_MIN, I32_MAX]))
            ri[i, e] = (v0, v1)
        for e in range(nsn):
            pair = (int(s[i]) - 1, int(s[i])) if rng.random() < 0.5 else (int(s[i]), int(s[i]) - 1)
            if rng.random() < 0.03:
                pair = (int(rng.choice([int(s[i]) - 2, int(s[i]), int(s[i]) + 1, -1, I32_MIN])), int(s[i]))
            si[i, e] = pair + (int(rng.integers(2)), int(rng.integers(-5, 5)))
    return Batch((nv_max, nr_max, np_max, ns_max), bw_max, n_anchors, rule, counts, r_idx, p_idx, s_idx, drop, (rc, ri), (pc, npn), (sc, si))


def test_random_windows_around_every_bound(driver, tmp_path):
    seen_all = np.zeros(10, dtype=int)
    for k, rule in enumerate(PAIR_RULE):
        rng = np.random.default_rng(20241019 + k)
        batches = [_random_batch(rng, rule) for _ in range(15)]
        assert sum(b.B for b in batches) >= 480
        seen = np.bincount(_check(driver, tmp_path, batches, "random_" + rule), minlength=10)
        print(f"{rule}: windows per code 0 .. 9:", seen.tolist())
        assert seen[0] > 0 and (seen[9] > 0) == (rule != "chain"), (rule, seen)
        seen_all += seen
    assert (seen_all[[0, 1, 2, 3, 4, 5, 6, 8, 9]] > 0).all() and seen_all[7] == 0, seen_all
