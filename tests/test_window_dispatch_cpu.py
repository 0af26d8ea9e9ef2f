"""localization_amd/csrc/window_dispatch.cpp on the CPU: which solve kernel a batch takes under every switch, and when the resident batch's
covariance verdict is served or thrown away.

tests/host/window_dispatch_driver.cpp (its own main; window_dispatch.cpp and window_structure.cpp compiled from source, nothing else of the
product, no HIP call) is built with g++ under AddressSanitizer + UBSan and run as a program on the full grids below.  A non-zero exit
status or anything on stderr fails the case.

The expected values, tests/golden/window_dispatch_table.npz, are a RECORDING of the code before the rules moved (commit c119a71, where they
were static functions of capi_window.cpp that took the handle): a scratch program held that commit's pick_kernel, effective_chain_min,
tree_min_batch, arrow3_wanted, cov_switches, the refused() lambda of loc_window_joint_covariance_resident and the two statements after it
that reset resident_cov to -1, bodies verbatim, behind a stand-in struct with the fields they read (the two *_lds_bytes calls answered by
the grid's "fits" columns); it read the same input file and wrote the same output as the driver.  The file holds that output and, as a
guard against a grid that drifts from the recording, the grids' axes.  A covariance verdict travels as CovKind's value; the scratch
program mapped it to the integers the parent kept in loc_window::resident_cov (-1, 0, 3, 6, 7, 8, 9, 10).

Rule set 3, what a resident entry refuses by the handle's state (resident_refusal), is held in the same way to tests/golden/window_refusal_table.npz:
a recording of commit 7061161, where every resident entry of capi_window.cpp spelled its refusals out.  The scratch program held that commit's
slide_check_handle, message_check_handle, check_pinfo_covers_resident and the heads of loc_window_solve_resident, loc_window_download,
loc_window_joint_covariance_resident, resident_audit_launch, resident_records_launch (with its two callers' argument checks in front),
loc_window_push_messages_resident_dev and loc_window_download_tables, bodies verbatim, behind a stand-in struct with the fields they read
(resident_topology answered by the grid's topology column, the condition of an entry's k-th argument check by "arg_failed == k"); it wrote the
return code and the text handed to locamd_fail for every row.  The grid is the full product of the axes below but for the rows no handle can be
in (pinfo_short without has_pinfo) and the argument checks an entry does not have; topology takes every LOC_WINDOW_KERNEL_* value."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "localization_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "window_dispatch_table.npz")
GOLDEN_REFUSAL = os.path.join(ROOT, "tests", "golden", "window_refusal_table.npz")
FLAGS = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]

# rule set 1: LOC_WINDOW_KERNEL_* (include/localization_amd.h) and the switches pick_kernel reads.  LOCAMD_CHAIN_MIN_BATCH, where set, is 4 096
# (so that n meets the threshold exactly on both rules, the default's 12 288 and an explicit one)
SOLVE_AXES = {
    "topology": list(range(9)),
    "n": [1, 255, 256, 4095, 4096, 12287, 12288, 65536],
    "chain_min": [-1, 0, 100, 5000],
    "env_chain_min_set": [0, 1],
    "has_off1": [0, 1], "natural_order": [0, 1], "wave3": [0, 1], "wave6": [0, 1], "chain3": [0, 1],
    "tree": [-1, 0, 2],
    "wave3_fits": [0, 1],
}
SOLVE_RESULTS = ("pick_kernel", "effective_chain_min", "tree_min_batch")
# rule set 2: CovKind Unclassified .. Envelope and what the admission and re-classification rules read (chain_min as created: the forest threshold is 256)
COV_AXES = {
    "kind": list(range(-1, 7)),
    "has_off1": [0, 1], "nv_max": [64, 65], "n": [255, 256], "tree": [-1, 0], "arrow3": [-1, 0, 1], "cov_general": [0, 1], "arrow_fits": [0, 1],
}
COV_RESULTS = ("cov_admitted", "cov_stale", "cov_stale_switches_changed", "cov_switches", "arrow3_wanted")
# rule set 3: ResidentEntry Solve .. DownloadTables, the facts of the handle and which of the entry's own argument checks fails first (0: none)
REFUSAL_AXES = {
    "entry": list(range(13)),
    "handle": [0, 1], "resident": [0, 1], "mirror_valid": [0, 1], "solved": [0, 1], "pinfo_short": [0, 1],
    "topology": list(range(9)),
    "has_off1": [0, 1], "has_pinfo": [0, 1], "pinfo_translation": [0, 1], "msg_set": [0, 1],
    "arg_failed": [0, 1, 2, 3, 4],
}
REFUSAL_ARGUMENT_CHECKS = [0, 0, 1, 1, 1, 1, 4, 3, 0, 1, 3, 3, 1]   # per entry


def solve_rows():
    rows = np.array(list(itertools.product(*SOLVE_AXES.values())), dtype=np.int64)
    env = np.where(rows[:, 3] == 1, 4096, 12288)                          # the env_chain_min column goes in after env_chain_min_set
    return np.concatenate([rows[:, :4], env[:, None], rows[:, 4:]], axis=1)


def cov_rows():
    return np.array(list(itertools.product(*COV_AXES.values())), dtype=np.int64)


def refusal_rows():
    rows = np.array(list(itertools.product(*REFUSAL_AXES.values())), dtype=np.int64)
    keep = (rows[:, 11] <= np.array(REFUSAL_ARGUMENT_CHECKS)[rows[:, 0]]) & ~((rows[:, 5] == 1) & (rows[:, 8] == 0))
    return rows[keep]


def write_refusal_table(path):
    rows = refusal_rows()
    with open(path, "wb") as f:
        np.array([3, rows.shape[0], rows.shape[1]], dtype=np.int64).tofile(f)
        np.ascontiguousarray(rows).tofile(f)


def read_refusals(out_path, texts_path):
    with open(texts_path, "rb") as f:
        texts = f.read().decode("utf-8").split("\n")
    assert texts[-1] == ""
    return np.fromfile(out_path, dtype=np.int64), texts[:-1]


def write_tables(path):
    with open(path, "wb") as f:
        for rule, rows in ((1, solve_rows()), (2, cov_rows())):
            np.array([rule, rows.shape[0], rows.shape[1]], dtype=np.int64).tofile(f)
            np.ascontiguousarray(rows).tofile(f)


def read_results(path):
    flat = np.fromfile(path, dtype=np.int64)
    n1 = len(solve_rows()) * len(SOLVE_RESULTS)
    assert flat.size == n1 + len(cov_rows()) * len(COV_RESULTS), flat.size
    return flat[:n1].reshape(-1, len(SOLVE_RESULTS)), flat[n1:].reshape(-1, len(COV_RESULTS))


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    d = tmp_path_factory.mktemp("window_dispatch_driver")
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("a sanitized program cannot be compiled and linked: no g++")
    rocm = os.path.dirname(os.path.dirname(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")))
    src = [os.path.join(ROOT, "tests", "host", "window_dispatch_driver.cpp"), os.path.join(CSRC, "window_dispatch.cpp"), os.path.join(CSRC, "window_structure.cpp")]
    # (the sanitizer runtimes linked INTO the program where the compiler has them as archives, as tests/test_window_structure_cpu.py does)
    for extra in (["-static-libasan", "-static-libubsan"], []):
        r = subprocess.run([cxx, "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), "-I", CSRC, "-pthread", *FLAGS, *extra, *src,
                            "-o", str(d / "driver")], capture_output=True, text=True)
        if r.returncode == 0:
            break
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]
    write_tables(d / "in.bin")
    r = subprocess.run([str(d / "driver"), str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-4000:])
    solve, cov = read_results(d / "out.bin")
    write_refusal_table(d / "in3.bin")
    r = subprocess.run([str(d / "driver"), str(d / "in3.bin"), str(d / "out3.bin"), str(d / "texts3.txt")], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-4000:])
    return {"solve": solve, "cov": cov, "golden": np.load(GOLDEN), "refusal": read_refusals(d / "out3.bin", d / "texts3.txt"), "refusal_golden": np.load(GOLDEN_REFUSAL)}


def assert_same(got, want, rows, names, columns):
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (f"{bad.size} of {len(rows)} rows differ; the first: " + ", ".join(f"{k}={v}" for k, v in zip(columns, rows[bad[0]].tolist())) +
                           " gives " + ", ".join(f"{k}={g} (recorded {w})" for k, g, w in zip(names, got[bad[0]].tolist(), want[bad[0]].tolist())))


def test_the_recording_is_of_these_grids(tables):
    g = tables["golden"]
    for prefix, axes in (("solve_", SOLVE_AXES), ("cov_", COV_AXES)):
        for name, values in axes.items():
            assert g[prefix + "axis_" + name].tolist() == values, name
    assert g["solve"].shape == (len(solve_rows()), 3) and g["cov"].shape == (len(cov_rows()), 5)
    assert len(solve_rows()) == 9 * 8 * 4 * 2 * 2 ** 5 * 3 * 2 and len(cov_rows()) == 8 * 2 ** 4 * 3 * 2 ** 2
    # every kernel is in the recording (TREE_LANE only as the topology handed through), and both answers of every covariance rule
    assert sorted(set(g["solve"][:, 0].tolist())) == list(range(9))
    assert all(sorted(set(g["cov"][:, k].tolist())) == [0, 1] for k in (0, 1, 2, 4))


def test_solve_kernel_table(tables):
    columns = list(SOLVE_AXES)[:4] + ["env_chain_min"] + list(SOLVE_AXES)[4:]
    assert_same(tables["solve"], tables["golden"]["solve"], solve_rows(), SOLVE_RESULTS, columns)


def test_resident_covariance_table(tables):
    assert_same(tables["cov"], tables["golden"]["cov"], cov_rows(), COV_RESULTS, list(COV_AXES))


def test_the_refusal_recording_is_of_this_grid(tables):
    g = tables["refusal_golden"]
    for name, values in REFUSAL_AXES.items():
        assert g["axis_" + name].tolist() == values, name
    assert g["argument_checks"].tolist() == REFUSAL_ARGUMENT_CHECKS
    rows = refusal_rows()
    assert len(rows) == (13 + sum(REFUSAL_ARGUMENT_CHECKS)) * 2 ** 9 * 9 * 3 // 4 and g["code"].shape == g["text"].shape == (len(rows),)
    # every code the entries return and every text of the parent is in the recording; "go on" has no text
    assert sorted(set(g["code"].tolist())) == [-5, -1, 0] and set(g["text"].tolist()) == set(range(len(g["texts"])))
    assert ((g["code"] == 0) == (g["texts"][g["text"]] == "")).all()


def test_resident_refusal_table(tables):
    g = tables["refusal_golden"]
    code, texts = tables["refusal"]
    rows = refusal_rows()
    want = g["texts"][g["text"]].tolist()
    assert len(code) == len(texts) == len(rows)
    bad = [i for i in range(len(rows)) if code[i] != g["code"][i] or texts[i] != want[i]]
    assert not bad, (f"{len(bad)} of {len(rows)} rows differ; the first: " + ", ".join(f"{k}={v}" for k, v in zip(REFUSAL_AXES, rows[bad[0]].tolist())) +
                     f" gives {code[bad[0]]} {texts[bad[0]]!r} (recorded {g['code'][bad[0]]} {want[bad[0]]!r})")
