"""Option "upload_dev_forest_groups" on the CPU, under host sanitizers: what loc_window_upload_dev relies on when it groups a mixed forest batch
on the device (window_groups_kernel.hip) and builds the groups block from the representatives alone.

tests/host/upload_dev_forest_groups_driver.cpp (its own main, window_structure.cpp compiled from source, nothing else of the product, no HIP
call) is built with g++ under AddressSanitizer + UBSan and run as a program of its own.  A non-zero exit status or anything on stderr fails
the case.  Held here:

1. window_groups.h's key, word by word, and its equality predicate against tests/_forest_groups_model.py's topology_key;
2. a serial model of the device rule on window_groups.h's hash (hash -> lowest window per hash -> verify -> number) against part (a) of
   build_tree_groups (group_windows), with the hash masked to 0, 2, 3 and 64 bits: without a collision the same of[] and rep[], and a
   collision is reported whenever windows of different keys share a masked hash;
3. part (b) (build_tree_groups_block) from the compact batch of the representatives + of[]: h_groups byte for byte build_tree_groups' on the
   full batch, and every refusal of build_tree_groups refused;
4. chain_scan(ordered = false) on the representatives = on the full batch (loc_window_upload_dev takes groups_no_chain from the former).

No tolerance anywhere: integers and bytes."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _forest_groups_model as F
import _window_structure_model as M
from _window_structure_model import Batch
from test_forest_groups_cpu import BASE, CAPS, mixed, star

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "localization_amd", "csrc")
FLAGS = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
BITS = (0, 2, 3, 64)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("upload_dev_forest_groups_driver")
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("a trivial sanitized program cannot be compiled and linked: no g++")
    trivial = d / "trivial.cpp"
    trivial.write_text("int main() { return 0; }\n")
    for extra in (["-static-libasan", "-static-libubsan"], []):
        r = subprocess.run([cxx, "-std=c++17", *FLAGS, *extra, str(trivial), "-o", str(d / "trivial")], capture_output=True, text=True)
        if r.returncode == 0:
            break
    else:
        pytest.skip(f"a trivial sanitized program cannot be compiled and linked ({' '.join(FLAGS)}): {r.stderr[-300:]}")
    rocm = os.path.dirname(os.path.dirname(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")))
    src = [os.path.join(ROOT, "tests", "host", "upload_dev_forest_groups_driver.cpp"), os.path.join(CSRC, "window_structure.cpp")]
    r = subprocess.run([cxx, "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), "-I", CSRC, "-pthread", *FLAGS, *extra, *src, "-o", str(d / "driver")],
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    return str(d / "driver")


def run(driver, tmp_path, batches):
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        for b in batches:
            b.write(f)
    r = subprocess.run([driver, str(src), str(dst), *(str(k) for k in BITS)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-4000:])
    out = M.read_sections(dst)
    assert len(out) == len(batches) and all(int(o["check"][0]) == 0 for o in out)
    return out


def check(b, o):
    """everything the driver reports for batch b; returns the number of groups (0: refused)"""
    n = b.n
    keys = [F.topology_key(b, i) for i in range(n)]
    # 1. the key, word by word, and the predicate
    at = o["key_at"].tolist()
    for i in range(n):
        assert tuple(o["keys"][at[i]:at[i + 1]].tolist()) == keys[i], i
    if "equal" in o:
        want = np.array([[keys[i] == keys[j] for j in range(n)] for i in range(n)], dtype=np.int32)
        assert np.array_equal(o["equal"].reshape(n, n), want)
    # the grouping by first appearance, whatever nv is
    ids, of, rep = {}, [], []
    for i, k in enumerate(keys):
        if k not in ids:
            ids[k] = len(rep)
            rep.append(i)
        of.append(ids[k])
    bad_nv = any(not 2 <= int(nv) <= 64 for nv in b.counts[:, 0])
    # part (a)
    assert int(o["a_ok"][0]) == (not bad_nv)
    if not bad_nv:
        assert o["a_of"].tolist() == of and o["a_rep"].tolist() == rep
    # 2. the model of the device rule
    for bits in BITS:
        fl = o[f"m_flags_{bits}"].tolist()
        assert fl[0] == bits and fl[1] == int(bad_nv) and fl[3] == 0, fl
        if bits == 64:
            assert fl[2] == 0
        if bits == 0:
            assert fl[2] == int(len(rep) > 1)                                  # every window collides with window 0
        if fl[2] == 0:
            assert fl[4] == len(rep) and o[f"m_of_{bits}"].tolist() == of and o[f"m_rep_{bits}"].tolist() == rep, bits
        else:
            assert fl[4] < len(rep)                                            # windows of different keys shared a hash: fewer candidates than groups
    # 3. part (b) against build_tree_groups
    want = F.groups(b)
    full, part = o["full"].tolist(), o["part_b"].tolist()
    assert full[0] == int(want is not None) and part == full, (full, part, want is not None)
    assert o["part_b_block"].tobytes() == o["full_block"].tobytes()
    if want is None:
        assert full[1] == 0 and len(o["part_b_block"]) == 0
        return 0
    assert full[1] == len(rep) and o["full_block"][full[2]:full[2] + n].tolist() == of
    # 4. the representatives answer for the batch
    chain = M.chain_scan(b, False)[0]
    assert o["chain"].tolist() == [int(chain), int(chain)]
    return len(rep)


FIVE = [BASE, dict(BASE, nv=24, every=3, flip=(3, 6), priors=(1, 5)), dict(BASE, nv=40, every=6, parent_of={7: 0}), dict(nv=2, every=1, priors=(1,)), dict(BASE, nv=33, every=5, robust=1)]


def test_five_topologies_every_window_its_own_and_one_topology(driver, tmp_path):
    five = mixed(70, [dict(k, anchor=a) for a in range(3) for k in FIVE][:15])                  # window b is of topology b % 5, other anchors per round
    assert [F.topology_key(five, i) == F.topology_key(five, i % 5) for i in range(70)] == [True] * 70
    back = Batch(70, n_anchors=5, **CAPS)                                                     # the topologies do not first appear in index order
    for i in range(70):
        star(back, i, **FIVE[4 - i % 5])
    last = Batch(70, n_anchors=5, **CAPS)                                                     # window B - 1 opens a group
    for i in range(70):
        star(last, i, **FIVE[4 if i == 69 else i % 4])
    own = Batch(63, n_anchors=5, **CAPS)                                                      # G = B: nv from 2 to 64
    for i in range(63):
        star(own, i, nv=2 + i, every=5, anchor=i % 5)
    one = mixed(70, [dict(FIVE[2], anchor=a, robust=a % 2) for a in range(5)])                # G = 1: other anchors and flags per window
    same = mixed(70, [FIVE[2]])                                                               # a true one-topology batch
    out = run(driver, tmp_path, [five, back, last, own, one, same])
    assert [check(b, o) for b, o in zip((five, back, last, own, one, same), out)] == [5, 5, 5, 63, 1, 1]
    assert out[1]["a_of"][:5].tolist() == [0, 1, 2, 3, 4] and out[1]["a_rep"].tolist() == [0, 1, 2, 3, 4]
    assert out[2]["a_rep"].tolist() == [0, 1, 2, 3, 69]


def test_fixed_endpoints_and_robust_flags_are_not_part_of_the_key(driver, tmp_path):
    anchors = mixed(6, [dict(BASE, anchor=a) for a in range(3)])
    robust = mixed(6, [dict(BASE, robust=r) for r in (0, 1)])
    out = run(driver, tmp_path, [anchors, robust])
    assert [check(b, o) for b, o in zip((anchors, robust), out)] == [1, 1]
    assert (anchors.r_idx[0, :9, 1] != anchors.r_idx[1, :9, 1]).all() and robust.s_idx[0, 0, 2] != robust.s_idx[1, 0, 2]
    for o in out:
        at = o["key_at"].tolist()
        assert all(o["keys"][at[i]:at[i + 1]].tolist() == o["keys"][:at[1]].tolist() for i in range(6))
        assert o["equal"].all()


def test_random_batches(driver, tmp_path):
    """random stars, random forests with pose-to-pose ranges in either direction, priors, EdgeSE3 in either direction"""
    rng = np.random.default_rng(8)
    batches = []
    for _ in range(10):
        kinds = [dict(nv=int(rng.integers(2, 65)), every=int(rng.integers(1, 9)), anchor=int(rng.integers(5)), robust=int(rng.integers(2)),
                      flip=tuple(int(x) for x in rng.integers(1, 64, 3)), priors=tuple(int(x) for x in rng.integers(0, 2, int(rng.integers(0, 3)))))
                 for _ in range(int(rng.integers(1, 7)))]
        b = Batch(int(rng.integers(1, 60)), n_anchors=5, **CAPS)
        for i in range(b.n):
            star(b, i, **kinds[int(rng.integers(len(kinds)))])
        batches.append(b)
    for _ in range(4):
        b = Batch(int(rng.integers(2, 30)), n_anchors=5, **CAPS)
        shapes = []
        for _ in range(3):
            nv = int(rng.integers(3, 30))
            shapes.append((nv, [(int(rng.integers(0, k)), k, int(rng.integers(3))) for k in range(1, nv) if rng.random() < 0.9]))
        for i in range(b.n):
            nv, edges = shapes[int(rng.integers(3))]
            for k in range(nv):
                b.add_pose(i)
            for u, v, how in edges:
                if how == 0:
                    b.add_se3(i, u, v, robust=int(rng.integers(2)))
                elif how == 1:
                    b.add_se3(i, v, u)
                else:
                    b.add_range(i, v, u)
            for k in range(nv):
                b.add_range(i, k, -1 - int(rng.integers(5)))
            b.add_prior(i, nv - 1)
        batches.append(b)
    out = run(driver, tmp_path, batches)
    assert all(check(b, o) >= 1 for b, o in zip(batches, out))


def test_every_refusal_of_build_tree_groups_is_refused(driver, tmp_path):
    good = mixed(7, [BASE, dict(BASE, nv=12, every=3)])
    cyc = good.copy("counts", "r_idx", "r_val")
    cyc.add_range(5, 1, 2)                                                    # a triangle in ONE window
    one = Batch(3, n_anchors=5, **CAPS)
    star(one, 0, **BASE); star(one, 1, nv=1, every=4); star(one, 2, **BASE)   # nv = 1
    wide = Batch(3, n_anchors=5, **dict(CAPS, nv_max=65, nr_max=70, ns_max=64))
    star(wide, 0, **BASE); star(wide, 1, nv=65, every=8); star(wide, 2, **BASE)   # nv = 65
    dbl = good.copy("counts", "s_idx", "s_val")
    dbl.add_se3(6, 0, 1)                                                      # a second EdgeSE3 on one pair
    off1 = good.copy(); off1.has_off1 = True
    long_handle = Batch(2, n_anchors=5, **dict(CAPS, nv_max=65))
    star(long_handle, 0, **BASE); star(long_handle, 1, **dict(BASE, nv=8))
    dbl_r = good.copy("counts", "r_idx", "r_val")
    dbl_r.add_range(6, 0, 1)                                                  # a doubled RANGE on a pair is no refusal
    batches = [good, cyc, one, wide, dbl, off1, long_handle, dbl_r]
    out = run(driver, tmp_path, batches)
    assert [check(b, o) for b, o in zip(batches, out)] == [2, 0, 0, 0, 0, 0, 0, 3]


def test_chain_verdict_from_the_representatives(driver, tmp_path):
    """windows that are chains in some edge order (every = 1: pose k hangs on k - 1) of two lengths: a grouped batch whose covariances the
    chain pass serves; one star among them: no chain"""
    chains = mixed(9, [dict(nv=9, every=1), dict(nv=6, every=1, anchor=2)])
    broken = mixed(9, [dict(nv=9, every=1), dict(nv=6, every=1), BASE])
    out = run(driver, tmp_path, [chains, broken])
    assert [check(b, o) for b, o in zip((chains, broken), out)] == [2, 3]
    assert out[0]["chain"].tolist() == [1, 1] and out[1]["chain"].tolist() == [0, 0]
