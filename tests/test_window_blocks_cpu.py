"""The block layouts of localization_amd/csrc/window_tables.h (covariance_layout, marginal_prior_layout, resident_pairs_layout,
slide_inputs_layout, slide_marginal_layout) and window_structure.cpp's max_anchor_referenced, on the CPU.

tests/host/window_blocks_driver.cpp (its own main; window_tables.h and window_structure.cpp compiled from source, nothing else of the product,
no HIP call) is built with g++ under AddressSanitizer + UBSan and run as a program.  A non-zero exit status or anything on stderr fails the
case.

The expected offsets, tests/golden/window_blocks_table.npz, are a RECORDING of the arithmetic the layout functions replaced (commit ff69eef,
where capi_window.cpp spelled each block by hand): a scratch program held that commit's expressions verbatim — the pre_bytes arrays of
loc_window_joint_covariance_host and loc_window_marginal_prior_host in front of that commit's pack_block, cnt_bytes / pair_bytes of
loc_window_joint_covariance_resident, piece[7] / at[8] of loc_window_slide_resident and slide_allocate's SlideBlock (mi, prior, grad, shift,
end; the drop table at 0, slot, rank and status at mi, 2 mi and 3 mi) — read the same input file and wrote the same output as the driver.
The file holds that output and, as a guard against a grid that drifts from the recording, the grid's axes.

Every offset must equal the recording.  One end may differ: the hand-written pair table was cnt_bytes + pair_bytes, its last piece not
rounded up; the layout's end is that rounded up to 16 bytes (the size of one allocation and one copy, no offset)."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "localization_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "window_blocks_table.npz")
FLAGS = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]

# N (and the handle's B for the slide's marginal block): at 1, 3 and 5 the int32 pieces are no multiples of 16 bytes
AXES = {
    "N": [1, 3, 4, 5, 65],
    "nv_max": [1, 10], "nr_max": [0, 19], "np_max": [0, 1, 3], "ns_max": [0, 2],
    "npair_max": [0, 1, 3], "nr_new_max": [0, 2], "np_new_max": [0, 1],
}
# the driver's 50 results per row: (block, prefix pieces, the eight tables follow)
BLOCKS = (("covariance", 6, True), ("marginal_prior", 7, True), ("resident_pairs", 2, False), ("slide_inputs", 7, False), ("slide_marginal", 7, False))
WIDTH = sum(n + (8 if tables else 0) + 1 for _, n, tables in BLOCKS)
PAIRS_END = 15 + 16 + 2   # the column of the pair table's end

I32_MIN = np.iinfo(np.int32).min


def grid_rows():
    return np.array(list(itertools.product(*AXES.values())), dtype=np.int64)


def anchor_batches():
    """ragged batches (counts [n][4], r_idx [n][nr_max][2]): counts below the capacity, and in the unused rows INT32_MIN — reading one as v1
    changes the answer, and negating it is an overflow UBSan stops at"""
    rng = np.random.default_rng(4711)
    out = []
    for n, nr_max, top in ((1, 1, 1), (3, 4, 6), (7, 19, 40), (64, 5, 3), (5, 3, 0), (4, 0, 0), (6, 8, 2000000)):
        counts = np.zeros((n, 4), dtype=np.int32)
        counts[:, 0] = rng.integers(1, 9, n)
        counts[:, 1] = rng.integers(0, nr_max + 1, n) if nr_max else 0
        if n > 2 and nr_max:
            counts[0, 1], counts[1, 1] = 0, nr_max   # an empty window and a full one
        r_idx = np.full((n, nr_max, 2), I32_MIN, dtype=np.int32)
        for i in range(n):
            for e in range(counts[i, 1]):
                anchor = top > 0 and rng.random() < 0.6
                r_idx[i, e] = (rng.integers(0, counts[i, 0]), -1 - rng.integers(0, top) if anchor else rng.integers(0, counts[i, 0]))
        out.append((counts, r_idx))
    return out


def max_anchor_numpy(counts, r_idx):
    used = np.arange(r_idx.shape[1])[None, :] < counts[:, 1:2]
    v1 = r_idx[:, :, 1][used].astype(np.int64)
    return int(max(0, (-v1[v1 < 0]).max(initial=0)))


def write_input(path):
    with open(path, "wb") as f:
        rows = grid_rows()
        np.array([1, rows.shape[0], rows.shape[1]], dtype=np.int64).tofile(f)
        np.ascontiguousarray(rows).tofile(f)
        for counts, r_idx in anchor_batches():
            np.array([2, r_idx.shape[0], r_idx.shape[1]], dtype=np.int64).tofile(f)
            np.ascontiguousarray(counts).tofile(f)
            np.ascontiguousarray(r_idx).tofile(f)


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    d = tmp_path_factory.mktemp("window_blocks_driver")
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("a sanitized program cannot be compiled and linked: no g++")
    rocm = os.path.dirname(os.path.dirname(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")))
    src = [os.path.join(ROOT, "tests", "host", "window_blocks_driver.cpp"), os.path.join(CSRC, "window_structure.cpp")]
    # (the sanitizer runtimes linked INTO the program where the compiler has them as archives, as tests/test_window_structure_cpu.py does)
    for extra in (["-static-libasan", "-static-libubsan"], []):
        r = subprocess.run([cxx, "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), "-I", CSRC, "-pthread", *FLAGS, *extra, *src,
                            "-o", str(d / "driver")], capture_output=True, text=True)
        if r.returncode == 0:
            break
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]
    write_input(d / "in.bin")
    r = subprocess.run([str(d / "driver"), str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-4000:])
    flat = np.fromfile(d / "out.bin", dtype=np.int64)
    n1 = len(grid_rows()) * WIDTH
    assert flat.size == n1 + len(anchor_batches()), flat.size
    return {"layouts": flat[:n1].reshape(-1, WIDTH), "anchors": flat[n1:], "golden": np.load(GOLDEN)}


def column_names():
    tables = ("poses", "counts", "r_val", "p_val", "s_val", "r_idx", "p_idx", "s_idx")
    out = []
    for block, n, with_tables in BLOCKS:
        out += [f"{block}.pre[{k}]" for k in range(n)] + ([f"{block}.tab[{t}]" for t in tables] if with_tables else []) + [f"{block}.end"]
    return out


def test_the_recording_is_of_this_grid(results):
    g = results["golden"]
    for name, values in AXES.items():
        assert g["axis_" + name].tolist() == values, name
    assert WIDTH == 50 and g["layouts"].shape == (len(grid_rows()), WIDTH) and len(grid_rows()) == 5 * 2 * 2 * 3 * 2 * 3 * 2 * 2
    assert column_names()[PAIRS_END] == "resident_pairs.end"
    # the recording has pieces that end off a 16-byte boundary (the alignment is exercised), and pair tables whose last piece does
    assert (g["layouts"][:, PAIRS_END] % 16 != 0).any()


def test_every_offset_is_the_recorded_one(results):
    got, want, rows, names = results["layouts"], results["golden"]["layouts"], grid_rows(), column_names()
    exact = np.arange(WIDTH) != PAIRS_END
    bad = np.argwhere(got[:, exact] != want[:, exact])
    assert bad.size == 0, (f"{len(bad)} offsets differ; the first: " + ", ".join(f"{k}={v}" for k, v in zip(AXES, rows[bad[0][0]].tolist())) +
                           f" gives {np.array(names)[exact][bad[0][1]]} = {got[:, exact][tuple(bad[0])]} (recorded {want[:, exact][tuple(bad[0])]})")
    assert (got % 16 == 0).all()   # every piece of every block, and every end, 16-byte aligned


def test_the_pair_table_ends_within_one_alignment_of_the_recording(results):
    got, want = results["layouts"][:, PAIRS_END], results["golden"]["layouts"][:, PAIRS_END]
    assert (got >= want).all() and (got - want < 16).all() and (got % 16 == 0).all(), (got - want).max()
    assert np.array_equal(got, (want + 15) // 16 * 16)


def test_anchor_scan_reads_the_used_rows_alone(results):
    want = [max_anchor_numpy(c, r) for c, r in anchor_batches()]
    assert results["anchors"].tolist() == want
    assert 0 in want and max(want) > 1000000 and len(set(want)) >= 4   # no anchor at all, a large code, several answers
