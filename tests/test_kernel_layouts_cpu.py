"""The memory layouts of localization_amd/csrc/window_layouts.h — wave3_lm_kernel, wave6_lm_kernel, arrow3_lm_kernel (LDS and workspace),
window_lm_kernel (main arrays, structure tables, index tables, staged values, small-window records, root supernode, push arrays) and the
four covariance passes — with their predicates and fit rules, on the CPU.

tests/host/kernel_layouts_driver.cpp (its own main; window_layouts.h compiled from source, nothing else of the product, no HIP call) is
built with g++ under AddressSanitizer + UBSan and run as a program.  A non-zero exit status or anything on stderr fails every case.  The
driver itself checks the structure of every layout (arrays inside the total, aligned, pairwise disjoint, ints behind the doubles) and
writes every element of every array of a buffer of exactly the layout's size: see its head comment.

The expected values, tests/golden/kernel_layouts_table.npz, are a RECORDING of the arithmetic the layout functions replaced (commit 9e16ce4,
where every kernel walked a pointer through its arrays and a host function summed the same terms up again).  A scratch program held that
commit's text verbatim — w3_carve, w6_carve, the two carve blocks of arrow3_lm_kernel and the carve of window_lm_kernel run on made-up base
addresses; window_wave3_lds_bytes, window_wave6_lds_bytes, arrow3_lds_doubles, window_arrow3_workspace_doubles_dev, window_instance_doubles,
window_index_doubles, window_table_bytes, small_table_doubles, window_push_doubles, window_lds_bytes, window_workspace_doubles and the
predicates; the fit rules as loc_window_create, loc_window_lds_bytes, build_arrow_aux and the launchers spelled them; cov_layout,
forest_cov_layout, env_layout, arrow_cov_layout, arrow_cov_ws_doubles — read the same input file and wrote the same columns as the driver.
The file holds that output and, as a guard against a grid that drifts from the recording, the grid's axes.  Equality is exact: the fit
thresholds decide dispatch, so no end may move."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "localization_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "kernel_layouts_table.npz")
FLAGS = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]

# bw_max -1 stands for nv_max - 1 (every value is clipped to nv_max - 1, as loc_window_create does)
AXES = {
    "nv_max": [1, 2, 10, 63, 64, 65, 100, 512, 513, 1000],
    "bw_max": [0, 1, 3, -1],
    "nr_max": [0, 1, 19, 65, 900, 4000],
    "np_max": [0, 1, 3, 64],
    "ns_max": [0, 2, 64, 65],
    "nb_max": [1, 5, 7, 15, 16],   # (16: beyond the launcher's 15, the first border whose 3 nb_max rows need no padding to a tile of 16)
}
# beyond what loc_window_create admits (nv_max <= 4096): the only capacities at which the envelope pass and the workspace-mode window kernel
# do NOT fit — the predicates are functions of the capacities alone and are asked on both sides
EXTRA = [(40000, 0, 0, 0, 0, 1), (40000, 1, 19, 1, 2, 5)]

W3 = ["T", "rec", "ev", "fix", "pv", "eidx", "epos", "pidx", "bytes"]
W6 = ["pose", "rec", "prec", "ev", "fix", "pv", "sv", "eidx", "epos", "pidx", "ppos", "bytes"]
A3 = ["PK", "GZ", "C0", "S", "bB", "xB", "xsB", "RA", "FX", "TB", "red", "AN", "lds_bytes", "TT", "XS", "BB", "CS", "ws_bytes"]
WIN = (["Hs", "Ls", "diagL", "b", "x", "yrow", "pose", "bak", "rrec", "prec", "srec", "index_main", "Us", "As", "otask_ws", "main_bytes", "tables"] +
       ["t." + n for n in ("rowmask", "colmask", "scr", "pushw", "rowpre", "perm", "boff", "ioff", "lvl_col", "lvl_blk", "lvl_mode", "colorder", "dense_off", "dense", "otask",
                           "fb", "last", "bytes")] +
       ["index_in_lds", "index_at", "i.ilist", "i.shared", "i.r_idx", "i.p_idx", "i.s_idx", "i.bytes", "r_val", "p_val", "s_val", "recA", "recB", "rec_count", "recA_cap",
        "root", "root_bytes", "lds_bytes"])
PRED = ["sparse_path", "mask_words", "nnz_capacity", "index_in_lds", "root_lds_doubles"]
FITS = ["wave3_fits", "wave3_fits.pinfo", "wave6_fits", "wave6_fits.se3", "arrow3_fits", "window_fits.lds", "window_fits.ws", "window_arrays_in_lds", "loc_window_lds_bytes",
        "cov_chain_fits.6", "cov_chain_fits.3", "cov_forest_fits", "cov_arrow_fits", "cov_envelope_fits"]
COV = ["hd", "ho", "kb", "dg", "rrec", "prec", "srec", "ints", "ri", "pi", "si", "mk", "bytes"]
FCOV = ["hd", "ho", "kb", "dg", "rec", "ints", "ei", "mk", "nd", "ps", "bytes"]
ENV = ["sinv", "rec", "ints", "ei", "wc", "first", "off", "last", "list", "mk", "bytes"]
ACOV = ["hd", "ho", "dg", "cc", "ig", "rec", "ints", "ei", "cnt", "mk", "flag", "bytes", "ws_doubles"]
COLUMNS = ([f"wave3.{n}" for n in W3] + [f"wave3.pinfo.{n}" for n in W3] + [f"wave6.{n}" for n in W6] + [f"wave6.se3.{n}" for n in W6] + [f"arrow3.{n}" for n in A3] +
           [f"window.lds.{n}" for n in WIN] + [f"window.ws.{n}" for n in WIN] + PRED + FITS + [f"cov6.{n}" for n in COV] + [f"cov3.{n}" for n in COV] +
           [f"forest_cov.{n}" for n in FCOV] + [f"env_cov.{n}" for n in ENV] + [f"arrow_cov.{n}" for n in ACOV])
WIDTH = len(COLUMNS)


def grid_rows():
    """every second point of the product of the first five axes (the parity of a weighted index sum), nb_max cycling along; then EXTRA"""
    names = list(AXES)[:5]
    rows = []
    for idx in itertools.product(*(range(len(AXES[n])) for n in names)):
        i_nv, i_bw, i_nr, i_np, i_ns = idx
        if (i_nv + i_bw + i_nr + i_np + i_ns) % 2:
            continue
        nv = AXES["nv_max"][i_nv]
        bw = AXES["bw_max"][i_bw]
        bw = nv - 1 if bw < 0 else min(bw, nv - 1)
        nb = AXES["nb_max"][(i_nv + i_nr + i_ns // 2) % 5]
        rows.append((nv, bw, AXES["nr_max"][i_nr], AXES["np_max"][i_np], AXES["ns_max"][i_ns], nb))
    return np.array(rows + EXTRA, dtype=np.int64)


def write_input(path):
    rows = grid_rows()
    with open(path, "wb") as f:
        np.array(rows.shape, dtype=np.int64).tofile(f)
        np.ascontiguousarray(rows).tofile(f)


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    d = tmp_path_factory.mktemp("kernel_layouts_driver")
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("a sanitized program cannot be compiled and linked: no g++")
    rocm = os.path.dirname(os.path.dirname(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")))
    src = [os.path.join(ROOT, "tests", "host", "kernel_layouts_driver.cpp")]
    # (the sanitizer runtimes linked INTO the program where the compiler has them as archives, as tests/test_window_blocks_cpu.py does)
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
    assert flat.size == len(grid_rows()) * WIDTH, flat.size
    return {"table": flat.reshape(-1, WIDTH), "golden": np.load(GOLDEN)}


def col(table, name):
    return table[:, COLUMNS.index(name)]


def test_the_recording_is_of_this_grid(results):
    g = results["golden"]
    for name, values in AXES.items():
        assert g["axis_" + name].tolist() == values, name
    assert g["extra"].tolist() == [list(e) for e in EXTRA]
    assert np.array_equal(g["rows"], grid_rows())
    assert g["table"].shape == (len(grid_rows()), WIDTH) and g["columns"].tolist() == COLUMNS
    assert 1500 <= len(grid_rows()) <= 4000


def test_every_offset_and_total_is_the_recorded_one(results):
    got, want, rows = results["table"], results["golden"]["table"], grid_rows()
    bad = np.argwhere(got != want)
    assert bad.size == 0, (f"{len(bad)} values differ; the first: " + ", ".join(f"{k}={v}" for k, v in zip(AXES, rows[bad[0][0]].tolist())) +
                           f" gives {COLUMNS[bad[0][1]]} = {got[tuple(bad[0])]} (recorded {want[tuple(bad[0])]})")


def test_alignments(results):
    t = results["table"]
    for pre in ("window.lds.", "window.ws."):
        for name in ("rowmask", "colmask", "scr", "pushw"):   # the u64 mask tables, from the start of LDS
            v = col(t, pre + "t." + name)
            at = col(t, pre + "tables")[v >= 0] + v[v >= 0]
            assert (at % 8 == 0).all(), name
        for name in ("Hs", "Ls", "diagL", "b", "x", "yrow", "pose", "bak", "rrec", "prec", "srec", "index_main", "tables", "index_at", "r_val", "p_val", "s_val", "recB", "root"):
            v = col(t, pre + name)
            assert (v[v >= 0] % 8 == 0).all(), name
    recA = col(t, "window.lds.recA")
    assert (recA >= 0).any() and (recA[recA >= 0] % 16 == 0).all()
    # both outcomes of the 16-byte alignment step in front of the records: the staged values end on an odd and on an even double
    before = (col(t, "window.lds.s_val") + 48 * 8 * grid_rows()[:, 4])[recA >= 0]
    assert set((before % 16).tolist()) == {0, 8} and ((recA[recA >= 0] - before) == before % 16).all()


def test_the_grid_takes_every_branch(results):
    t, rows = results["table"], grid_rows()
    nv, bw, nr, np_, ns, nb = rows.T
    both = lambda v: set(np.unique(v).tolist()) == {0, 1}   # noqa: E731
    # SKYLINE against SPARSE at 512 / 513, one-word against eight-word masks at 64 / 65
    sp, words = col(t, "sparse_path"), col(t, "mask_words")
    assert sp[nv == 512].all() and not sp[nv == 513].any() and (words[nv == 64] == 1).all() and (words[nv == 65] == 8).all()
    # the bumped band of window_nnz_capacity: 65 .. 512 poses with bw_max < 3 get the capacity of bw_max = 3; nobody else
    nnz = col(t, "nnz_capacity")
    plain = np.array([sum(36 * (min(v, b) + 1) for v in range(n)) if n <= 1000 else 36 * (b + 1) * n - 36 * b * (b + 1) // 2 for n, b in zip(nv.tolist(), bw.tolist())])
    bumped = (nv > 64) & (nv <= 512) & (bw < 3)
    assert bumped.any() and (nnz[bumped] > plain[bumped]).all() and (nnz[~bumped] == plain[~bumped]).all()
    assert ((nv > 64) & (nv <= 512) & (bw >= 3)).any()
    # window_index_in_lds both ways under each of its two limits
    iil = col(t, "index_in_lds")
    assert both(iil[nv <= 64]) and both(iil[nv > 64])
    assert not iil[(nv == 10) & (nr >= 900)].any() and iil[(nv == 10) & (nr <= 65) & (ns <= 2)].all()
    assert both(col(t, "window.ws.index_in_lds")) and not col(t, "window.lds.index_in_lds").any()
    # the root supernode
    root = col(t, "root_lds_doubles")
    assert (root[words == 8] > 0).any() and (root[(words == 8) & (sp == 1)] == 0).any() and (root[words == 1] == 0).all()
    assert (col(t, "window.ws.root") >= 0).any() and (col(t, "window.lds.root") == -1).all()
    # global_a both ways where both are legal: windows of <= 64 poses whose arrays fit the LDS may run in either mode
    legal = (col(t, "window_arrays_in_lds") == 1) & (col(t, "window_fits.ws") == 1)
    assert legal.any() and both(col(t, "window_arrays_in_lds"))
    assert (col(t, "window.lds.recA")[legal] >= 0).all() and (col(t, "window.ws.recA") == -1).all()
    assert (col(t, "window.ws.Us")[sp == 1] >= 0).all() and (col(t, "window.ws.Us")[sp == 0] == -1).all() and (col(t, "window.lds.Us") == -1).all()
    assert (col(t, "window.ws.otask_ws")[words == 8] >= 0)[sp[words == 8] == 1].all() and (col(t, "window.ws.t.otask")[words == 1] >= 0).all()
    # wave3 with and without the dense prior records, wave6 with and without EdgeSE3 records; int counts odd and even
    assert (col(t, "wave3.pinfo.bytes") > col(t, "wave3.bytes")).any() and (col(t, "wave6.se3.sv") >= 0).all() and (col(t, "wave6.sv") == -1).all()
    # int counts odd and even: wave3 has 4 nr_max + np_max ints and rounds an odd count up; wave6 has 4 nr_max + 2 np_max, even whatever the capacities
    assert both((4 * nr + np_) % 2)
    w3_ints, w6_ints = col(t, "wave3.bytes") - col(t, "wave3.eidx"), col(t, "wave6.bytes") - col(t, "wave6.eidx")
    assert np.array_equal(w3_ints, 4 * (4 * nr + np_ + np_ % 2)) and np.array_equal(w6_ints, 4 * (4 * nr + 2 * np_))
    # arrow3: 3 nb_max a multiple of 16 and not (FX: 4 waves x 4 x D16 x 3 doubles, D16 = 3 nb_max rounded up to 16)
    d16 = (3 * nb + 15) // 16 * 16
    assert both(3 * nb % 16 == 0) and np.array_equal(col(t, "arrow3.TB") - col(t, "arrow3.FX"), 4 * 4 * d16 * 3 * 8)
    # each fit predicate on both sides of its limit
    for name in FITS:
        if name != "loc_window_lds_bytes":
            assert both(col(t, name)), name
