"""CPU-side checks behind the joint covariance calls (loc_window_joint_covariance_*; DESIGN.md §2, "Joint marginals"):
  * the identities the four passes form a cross block [H^-1]_ij with — numpy models (tests/_joint_cov_models.py) against np.linalg.inv
    at the oracle-solved poses of the GPU tests' inputs, to 1e-10 of sqrt(||R_ii|| ||R_jj||);
  * loc_window_joint_covariance_plan against the Python profile model with the pairs as edges, its equality with
    loc_window_covariance_plan without pairs, and its LOC_ERR_INVALID cases — no device;
  * check_pairs and envelope_blocks_max_joint of window_structure.cpp through a stand-alone driver (tests/host/joint_pairs_driver.cpp, its
    own main) built with g++ under AddressSanitizer + UBSan, on valid and invalid pairs with poisoned unused slots."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import localization_amd as la
from localization_amd.window import covariance_plan, joint_covariance_plan
import _general_cov_inputs as G
import _joint_cov_models as M
from _covariance_ref import hessian

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "localization_amd", "csrc")
I32_MIN, I32_MAX = np.iinfo(np.int32).min, np.iinfo(np.int32).max
LIMIT = 1e-10


def _solved_H(wb, i, anchors):
    """H of window i at its oracle-solved poses (numeric Jacobians), excluded diagonals 1, and the reference inverse"""
    from oracle import oracle as O
    from _oracle_window import oracle_solve_instance
    nv = int(wb.counts[i, 0])
    wb.poses[i, :nv] = oracle_solve_instance(wb, i, anchors, jac_mode=O.JAC_NUMERIC_G2O)[0]
    H = hessian(wb, i, anchors, O.JAC_NUMERIC_G2O)
    Sig, keep = M.kept_inverse(H)
    return M.unit_excluded(H), Sig, keep, nv


def _assert_block(got, Sig, keep, i, j, what):
    k_i, k_j = keep[6 * i:6 * i + 6], keep[6 * j:6 * j + 6]
    g = np.where(np.outer(k_i, k_j), got, 0.0)   # (the kernels write 0 in excluded rows / columns)
    err = M.block_error(g, Sig, i, j)
    assert err <= LIMIT, (what, i, j, err)
    return err


def _spread_pairs(nv):
    """adjacent in both orders, the ends, a diagonal, the middle against both ends"""
    if nv == 1:
        return [(0, 0)]
    return [(0, 1), (1, 0), (0, nv - 1), (nv - 1, 0), (nv // 2, nv // 2), (nv // 2, nv - 1), (0, nv // 2), (nv - 2, nv - 1)]


@pytest.mark.parametrize("kind", ["translation_10", "imu_lever_12", "twist_15"])
def test_chain_recipe(built, kind):
    from test_gpu_covariance import ANCH, _observable_batch, _twist_batch
    rng = np.random.default_rng(2024)
    if kind == "translation_10":
        wb = _observable_batch(la, rng, 3, 10, False, False, translation_only=True)
    elif kind == "imu_lever_12":
        wb = _observable_batch(la, rng, 3, 12, True, True)
    else:
        wb = _twist_batch(la, rng, 3, 15, True)
    for w in range(wb.B):
        H, Sig, keep, nv = _solved_H(wb, w, ANCH)
        for i, j in _spread_pairs(nv):
            _assert_block(M.chain_cross(H, nv, i, j), Sig, keep, i, j, kind)


def test_chain_recipe_with_a_missing_link(built):
    """window 2 of _observable_batch misses the link 2 - 3: two independent chains, exact zeros between them"""
    from test_gpu_covariance import ANCH, _observable_batch
    wb = _observable_batch(la, np.random.default_rng(2025), 3, 10, False, False, translation_only=True)
    H, Sig, keep, nv = _solved_H(wb, 2, ANCH)
    assert not M.blk(H, 3, 2).any() and M.blk(H, 2, 1).any()
    assert not M.chain_cross(H, nv, 1, 5).any() and not M.blk(Sig, 1, 5).any()
    _assert_block(M.chain_cross(H, nv, 3, 9), Sig, keep, 3, 9, "missing link")


@pytest.mark.parametrize("name", ["rich_10_1", "rich_24_4", "isolated_pose"])
def test_forest_recipe(built, name):
    from test_gpu_forest_covariance import ANCH, _case
    wb, _ = _case(la, name)
    T = wb.caps[0]
    for w in range(2):
        H, Sig, keep, nv = _solved_H(wb, w, ANCH)
        parent = M.forest_parents(nv, M.pose_pairs(wb, w))
        model = M.ForestModel(H, parent)
        roots = [v for v in range(nv) if parent[v] < 0]
        leaves = [v for v in range(nv) if v not in parent]
        pairs = [(leaves[0], parent[leaves[0]]), (parent[leaves[0]], leaves[0]), (leaves[0], leaves[-1]), (leaves[-1], leaves[1]), (0, nv - 1), (3, 3)]
        if name == "rich_24_4":      # two trees: poses 0 .. 14 and 15 .. 23
            assert len(roots) == 2
            pairs += [(2, 20), (14, 15)]
            assert not model.cross(2, 20).any() and not M.blk(Sig, 2, 20).any()
        if name == "isolated_pose":
            assert parent[T - 1] < 0 and T - 1 in leaves
            assert not model.cross(T - 1, 0).any() and not M.blk(Sig, T - 1, 0).any()
        for i, j in pairs:
            _assert_block(model.cross(i, j), Sig, keep, i, j, name)


@pytest.mark.parametrize("name", ["5_1", "24_4"])
def test_arrowhead_recipe(built, name):
    from _arrow_cov_inputs import SURVEYED, case_batch, ranged_nodes
    wb = case_batch(la, name)
    for w in range(3):
        H, Sig, keep, nv = _solved_H(wb, w, SURVEYED)
        nb = len(ranged_nodes(wb, w)[1])
        nc = nv - nb
        pairs = [(a, b) for a in range(nc, nv) for b in range(nc, nv)] + [(0, nc), (nv - 1, nc - 1), (0, 1), (1, 0), (0, nc - 1), (nc // 2, nc // 2), (nc - 1, 1)]
        for i, j in pairs:
            _assert_block(M.arrow_cross(H, nv, nb, i, j), Sig, keep, i, j, name)


def test_envelope_recipe(built):
    """the mixed batch with a pair outside every window's original envelope: the blocks the pairs add are exact zeros until true fill
    reaches them, and the selected inversion leaves [H^-1]_ij there"""
    wb = G.mixed_batch(la)
    for w in range(wb.B):
        H, Sig, keep, nv = _solved_H(wb, w, G.ANCH)
        first0 = G.envelope_first(nv, G.window_pairs(wb, w))
        outside = [(i, j) for i in range(nv) for j in range(i) if j < first0[i]]
        pairs = [(0, 1), (nv - 1, nv - 1)] + ([outside[0], outside[-1][::-1]] if outside else [])
        assert outside or w == 2     # (the key-first star's envelope is already full)
        W = M.envelope_inverse(H, G.envelope_first(nv, G.window_pairs(wb, w) + pairs))
        for i, j in pairs + [(v, v) for v in range(nv)]:
            _assert_block(M.envelope_cross(W, i, j), Sig, keep, i, j, ("mixed", w))


# ---- loc_window_joint_covariance_plan -----------------------------------------------------------------------------------------------
def test_plan_counts_the_pairs(built):
    wb = G.mixed_batch(la)
    assert joint_covariance_plan(wb, np.zeros((0, 2), dtype=np.int32)) == covariance_plan(wb)
    rng = np.random.default_rng(5)
    npm = 4
    pairs = np.full((wb.B, npm, 2), I32_MIN, dtype=np.int32)
    counts = np.array([4, 0, 2, 1, 3, 4], dtype=np.int32)
    for w in range(wb.B):
        nv = int(wb.counts[w, 0])
        pairs[w, :counts[w]] = rng.integers(0, nv, (counts[w], 2))
    pairs[0, 0] = (23, 0)                                   # the chain window: one whole row
    blocks, nbytes = joint_covariance_plan(wb, pairs, counts)
    per_window = [M.envelope_blocks_with_pairs(wb, w, pairs[w, :counts[w]]) for w in range(wb.B)]
    assert blocks == max(per_window) and per_window[0] >= 2 * 24 - 1 + 22
    assert nbytes == wb.B * ((blocks + 24) * 36 + 24 * 6) * 8
    # pairs inside the envelope (and no pairs at all) cost nothing
    assert joint_covariance_plan(wb, pairs, np.zeros(wb.B, dtype=np.int32)) == covariance_plan(wb)
    assert joint_covariance_plan(wb, [(1, 0), (0, 0), (1, 1)]) == covariance_plan(wb)
    # a window whose pairs make it the batch's largest
    chains = G.chain_batch(la, 1, 2, 65, False, ragged=False)
    assert covariance_plan(chains)[0] == 2 * 65 - 1
    assert joint_covariance_plan(chains, [(0, 64)])[0] == 2 * 65 - 1 + 63


def test_plan_refuses_bad_pairs(built):
    wb = G.mixed_batch(la)
    nv = [int(x) for x in wb.counts[:, 0]]

    def refused(pairs, counts=None, npm=None):
        with pytest.raises(la.LocalizationAmdError) as ex:
            joint_covariance_plan(wb, pairs, counts)
        assert ex.value.code == -1

    ok = np.zeros((wb.B, 2, 2), dtype=np.int32)
    joint_covariance_plan(wb, ok)
    for w, slot, v in ((4, (0, 0), nv[4]), (5, (1, 1), -1), (0, (1, 0), 24), (3, (0, 1), I32_MIN)):
        bad = ok.copy(); bad[w][slot] = v
        refused(bad)
        assert joint_covariance_plan(wb, bad, np.where(np.arange(wb.B) == w, slot[0], 2).astype(np.int32)) == covariance_plan(wb)   # (an unused slot is never read)
    refused(ok, np.array([2, 2, 3, 2, 2, 2], dtype=np.int32))
    refused(ok, np.array([2, 2, 2, 2, -1, 2], dtype=np.int32))


# ---- the host passes under AddressSanitizer + UBSan -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("joint_pairs_driver")
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    rocm = os.path.dirname(os.path.dirname(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")))
    src = [os.path.join(ROOT, "tests", "host", "joint_pairs_driver.cpp"), os.path.join(CSRC, "window_structure.cpp")]
    for extra in (["-static-libasan", "-static-libubsan"], []):   # (the runtimes linked into the program where the compiler has them as archives)
        r = subprocess.run([cxx, "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), "-I", CSRC, "-pthread", *flags, *extra, *src,
                            "-o", str(d / "driver")], capture_output=True, text=True)
        if r.returncode == 0:
            return str(d / "driver")
    raise AssertionError(r.stderr[-3000:])


def _write(f, caps, counts, r_idx, s_idx, pair_counts, pairs):
    n = len(counts)
    np.array(caps + (pairs.shape[1],), np.int32).tofile(f)
    np.array([n], np.int64).tofile(f)
    for a in (counts, r_idx, s_idx, pair_counts, pairs):
        np.ascontiguousarray(a, dtype=np.int32).tofile(f)


def _model(caps, counts, r_idx, s_idx, pair_counts, pairs):
    """(check_pairs, envelope_blocks_max_joint, envelope_blocks_max) as window_structure.h words them"""
    npm = pairs.shape[1]
    check, most, most_plain = 0, 0, 0
    bad_env = bad_plain = False
    for i in range(len(counts)):
        nv, nr, _, ns = (int(x) for x in counts[i])
        pc = int(pair_counts[i])
        mine = 0
        if npm > 0:
            if pc < 0 or pc > npm:
                mine = 1
            elif any(not (0 <= int(x) < nv) for x in pairs[i, :pc].ravel()):
                mine = 2
        check = check or mine
        edges = [(int(a), int(b)) for a, b in r_idx[i, :nr] if b >= 0] + [(int(a), int(b)) for a, b in s_idx[i, :ns, :2]]
        if any(not (0 <= a < nv and 0 <= b < nv) for a, b in edges) or any(not 0 <= int(a) < nv for a, b in r_idx[i, :nr]):
            bad_env = bad_plain = True
            continue
        most_plain = max(most_plain, int((np.arange(nv) - G.envelope_first(nv, edges) + 1).sum()))
        if mine:
            bad_env = True
            continue
        extra = [(int(a), int(b)) for a, b in pairs[i, :pc]] if npm > 0 else []
        most = max(most, int((np.arange(nv) - G.envelope_first(nv, edges + extra) + 1).sum()))
    return check, -1 if bad_env else most, -1 if bad_plain else most_plain


def test_pair_check_and_envelope_count_under_sanitizers(driver, tmp_path):
    rng = np.random.default_rng(77)
    caps = (12, 20, 6)
    batches = []

    def random_batch(n, npm):
        counts = np.zeros((n, 4), np.int32)
        r_idx = np.full((n, caps[1], 2), I32_MIN, np.int32)
        s_idx = np.full((n, caps[2], 4), I32_MAX, np.int32)
        pair_counts = np.zeros(n, np.int32)
        pairs = np.full((n, npm, 2), I32_MIN, np.int32)          # unused slots poisoned
        pairs[:, :, 1] = I32_MAX
        for i in range(n):
            nv = int(rng.integers(1, 13))
            nr = int(rng.integers(0, 21)) if nv > 1 else 0
            ns = int(rng.integers(0, 7)) if nv > 1 else 0
            counts[i] = (nv, nr, 0, ns)
            for e in range(nr):
                v0 = int(rng.integers(nv))
                r_idx[i, e] = (v0, -1 - int(rng.integers(2)) if rng.random() < 0.3 else int((v0 + rng.integers(1, nv)) % nv))
            for e in range(ns):
                v0 = int(rng.integers(nv))
                s_idx[i, e] = (v0, int((v0 + rng.integers(1, nv)) % nv), 0, 0)
            pair_counts[i] = int(rng.integers(0, npm + 1))
            pairs[i, :pair_counts[i]] = rng.integers(0, nv, (pair_counts[i], 2))
        return [counts, r_idx, s_idx, pair_counts, pairs]

    for _ in range(8):
        batches.append(random_batch(int(rng.integers(1, 6)), int(rng.integers(1, 7))))
    batches.append(random_batch(3, 0))                            # npair_max = 0: nothing is read
    batches.append(random_batch(4200, 3))                         # the threaded path
    n_valid = len(batches)
    base = random_batch(4, 5)
    base[3][:] = 5
    for i in range(4):
        base[4][i] = rng.integers(0, base[0][i, 0], (5, 2))
    batches.append(base)
    for w, count in ((0, 6), (3, -1), (2, I32_MAX), (1, I32_MIN)):            # a pair count outside [0, npair_max]
        b = [a.copy() for a in base]; b[3][w] = count; batches.append(b)
    for w, p, k, v in ((0, 0, 0, None), (3, 4, 1, None), (2, 2, 0, -1), (1, 4, 1, I32_MIN), (2, 0, 1, I32_MAX)):   # a slot outside [0, nv)
        b = [a.copy() for a in base]; b[4][w, p, k] = int(base[0][w, 0]) if v is None else v; batches.append(b)
    big = random_batch(4200, 3)
    big[3][4150] = 3; big[4][4150, 2, 1] = 12                    # one bad slot in the last thread's range
    batches.append(big)
    src = tmp_path / "in.bin"
    with open(src, "wb") as f:
        for b in batches:
            _write(f, caps, *b)
    r = subprocess.run([driver, str(src)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-4000:])
    got = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    want = [_model(caps, *b) for b in batches]
    assert got == want
    assert all(g[0] == 0 and g[1] >= g[2] > 0 for g in got[:n_valid + 1])
    assert [g[0] for g in got[n_valid + 1:]] == [1] * 4 + [2] * 6 and all(g[1] == -1 and g[2] > 0 for g in got[n_valid + 1:])
