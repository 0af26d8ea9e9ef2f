"""localization_amd/csrc/window_structure.cpp on the CPU, under host sanitizers: the validation that stands between a caller's index
tables and the kernels, the scans that pick the kernel and key the topology cache, and the two table builders whose output
tree_wave_kernel / tree_lm_kernel / forest_covariance_kernel / arrow3_lm_kernel index with unchecked.

tests/host/window_structure_driver.cpp (its own main, window_structure.cpp compiled from source, nothing else of the product, no
HIP call) is built twice with g++: AddressSanitizer + UBSan, and ThreadSanitizer.  Every case runs under the first build, the
batches of >= 4 096 instances (where the passes split over threads) under the second as well.  A non-zero exit status or anything
on stderr fails the case.  The expected values come from tests/_window_structure_model.py; unused table slots are poisoned."""
import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import _window_structure_model as M
from _window_structure_model import Batch, I32_MAX, I32_MIN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "localization_amd", "csrc")
SANITIZERS = {"asan": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "tsan": ["-O1", "-g", "-fsanitize=thread"]}
# the runtimes linked INTO the programs where the compiler has them as archives: a program then starts whatever else the loader is told to load first
STATIC = {"asan": ["-static-libasan", "-static-libubsan"], "tsan": ["-static-libtsan"]}


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("window_structure_driver")
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("a trivial sanitized program cannot be compiled and linked: no g++")
    trivial = d / "trivial.cpp"
    trivial.write_text("#include <thread>\nint main() { int x = 0; std::thread t([&x] { x = 1; }); t.join(); return x - 1; }\n")
    flags_of = {}
    for name, flags in SANITIZERS.items():
        for extra in (STATIC[name], []):
            r = subprocess.run([cxx, "-std=c++17", "-pthread", *flags, *extra, str(trivial), "-o", str(d / ("trivial_" + name))], capture_output=True, text=True)
            if r.returncode == 0:
                flags_of[name] = flags + extra
                break
        else:
            pytest.skip(f"a trivial sanitized program cannot be compiled and linked ({' '.join(flags)}): {r.stderr[-300:]}")
    rocm = os.path.dirname(os.path.dirname(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")))
    src = [os.path.join(ROOT, "tests", "host", "window_structure_driver.cpp"), os.path.join(CSRC, "window_structure.cpp")]
    procs = {name: subprocess.Popen([cxx, "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), "-I", CSRC, "-pthread", *flags, *src,
                                     "-o", str(d / name)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for name, flags in flags_of.items()}
    for name, p in procs.items():
        log = p.communicate()[0]
        assert p.returncode == 0, (name, log[-3000:])
    info = dict(line.split() for line in _clean_run([str(d / "asan"), "--info"]).splitlines())
    tsan_starts = ""                                                      # can the ThreadSanitizer runtime start here at all (a few times: the layout is random)
    for _ in range(4):
        r = subprocess.run([str(d / "trivial_tsan")], capture_output=True, text=True, preexec_fn=_no_aslr)
        if r.returncode != 0:
            tsan_starts = f"a trivial ThreadSanitizer program does not run here (exit status {r.returncode}): {r.stderr[-200:]}"
    return {"asan": str(d / "asan"), "tsan": str(d / "tsan"), "hw": int(info["hw"]), "lds": int(info["lds"]), "tsan_unusable": tsan_starts}


def _no_aslr():
    """ThreadSanitizer keeps its shadow memory at fixed addresses, and this compiler's runtime does not survive every randomised layout
    (kernels with 32 random mmap bits: "FATAL: ThreadSanitizer: unexpected memory mapping", or a crash before main).  Its programs
    therefore start with ADDR_NO_RANDOMIZE, a flag of the child process alone."""
    try:
        ctypes.CDLL(None).personality(0x0040000)
    except (OSError, AttributeError):
        pass


def _clean_run(cmd, preexec_fn=None):
    r = subprocess.run(cmd, capture_output=True, text=True, preexec_fn=preexec_fn)
    assert r.returncode == 0 and r.stderr == "", (cmd[0], r.returncode, r.stderr[-4000:])
    return r.stdout


def run(drivers, tmp_path, batches, tsan=False):
    """Every batch through the driver: the ASan + UBSan build, and the TSan build on request (the same answers are required of it)."""
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        for b in batches:
            b.write(f)
    _clean_run([drivers["asan"], str(src), str(dst)])
    out = M.read_sections(dst)
    assert len(out) == len(batches)
    if tsan:
        assert all(b.n >= 4096 for b in batches)
        if out[0]["batch"][1] <= 1:
            pytest.skip("the driver reports one hardware thread: the passes would not split, ThreadSanitizer would see nothing")
        if drivers["tsan_unusable"]:
            pytest.skip(drivers["tsan_unusable"])
        _clean_run([drivers["tsan"], str(src), str(dst)], preexec_fn=_no_aslr)
        again = M.read_sections(dst)
        for a, c in zip(out, again):
            assert a.keys() == c.keys() and all(np.array_equal(a[k], c[k]) for k in a if k != "check"), "the TSan build computes something else"
        out = [dict(a, check_tsan=c["check"]) for a, c in zip(out, again)]
    return out


def test_lds_formula_is_the_kernels(drivers):
    # arrow3_lds_layout(100, 7) (window_layouts.h) by hand: 2800 + 231 + 253 + 63 + 84 + 1536 + 42 + 16 + 768 = 5793 doubles
    assert drivers["lds"] == 46344 == M.arrow3_lds_bytes(100, 7)


# ---- small windows for the threaded passes --------------------------------------------------------------------------------------

SMALL_CAPS = dict(nv_max=4, nr_max=4, np_max=2, ns_max=2, bw_max=1)


@functools.lru_cache(maxsize=None)
def small_windows(n, seed=0, se3=True, chains=False):
    """n valid windows of 3 or 4 poses (never changed: variants copy the tables they edit).  Range edge 0 and SE3 edge 0 join pose 1
    to pose 0 or 2, so that ONE changed entry can stretch them.  chains: ordered chains with single pairs, translation-only."""
    rng = np.random.default_rng(seed + n)
    b = Batch(n, n_anchors=3, **SMALL_CAPS)
    for i in range(n):
        nv = 3 + int(rng.integers(2))
        for k in range(nv):
            b.add_pose(i, rng.normal(size=3))
        if chains:
            for k in range(nv):
                if k and rng.random() < 0.8:
                    b.add_range(i, *((k - 1, k) if rng.random() < 0.5 else (k, k - 1)))
                elif b.counts[i, 1] < 4 and rng.random() < 0.5:
                    b.add_range(i, k, -1 - int(rng.integers(3)))
            for k in sorted(rng.integers(0, nv, int(rng.integers(3))).tolist()):
                b.add_prior(i, k)
            continue
        b.add_range(i, 1, 2 * int(rng.integers(2)))
        for _ in range(int(rng.integers(1, 4))):
            v0 = int(rng.integers(nv))
            v1 = -1 - int(rng.integers(3)) if rng.random() < 0.4 else (v0 + 1 if v0 == 0 or (v0 < nv - 1 and rng.random() < 0.5) else v0 - 1)
            b.add_range(i, v0, v1, lever=(0.0, 0.1, 0.0))
        for _ in range(1 + int(rng.integers(2))):
            b.add_prior(i, int(rng.integers(nv)))
        if se3:
            b.add_se3(i, 1, 2 * int(rng.integers(2)))
            if rng.random() < 0.5:
                v0 = int(rng.integers(nv - 1))
                b.add_se3(i, v0 + 1, v0, robust=1)
    return b


def corrupt(base, i, code):
    """One entry of instance i changed so that check `code` fails (and no earlier one)."""
    nv = int(base.counts[i, 0])
    b = base.copy("counts", "r_idx", "p_idx", "s_idx")
    if code == 1:
        b.counts[i, i % 4] = base.caps[i % 4] + 1
    elif code == 2:
        b.r_idx[i, 0, 0] = nv
    elif code == 3:
        b.r_idx[i, 0, 0] = 2 - b.r_idx[i, 0, 1]     # pose 1 -> the pose two slots from the other end
    elif code == 4:
        b.p_idx[i, 0] = nv
    elif code == 5:
        b.s_idx[i, 0, 1] = nv
    else:
        b.s_idx[i, 0, 0] = 2 - b.s_idx[i, 0, 1]
    return b


@pytest.mark.parametrize("code", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("n", [1, 4095, 4096, 4099])
def test_check_instances_names_the_one_bad_entry(drivers, tmp_path, n, code):
    base = small_windows(n)
    ranges = M.thread_ranges(n, drivers["hw"])
    assert len(ranges) == (1 if n < 4096 else min(8, drivers["hw"]))
    where = sorted({0, n - 1} | {x for lo, hi in ranges if hi > lo for x in (lo, hi - 1)})
    batches = [base] + [corrupt(base, i, code) for i in where]
    for i, b in zip(where, batches[1:]):
        assert M.first_failed_check(b, i) == code
    out = run(drivers, tmp_path, batches, tsan=n >= 4096)
    for key in ("check",) + (("check_tsan",) if n >= 4096 else ()):
        assert out[0][key][0] == 0, key
        assert [int(o[key][0]) for o in out[1:]] == [code] * len(where), (key, where)
    assert "hash" in out[0] and "tsched" not in out[1]          # nothing but the guard and the envelope ran on the bad tables


def test_check_instances_base_batches_are_valid():
    for n in (1, 4095, 4099):
        b = small_windows(n)
        assert all(M.first_failed_check(b, i) == 0 for i in range(n))
        if n > 1:                                                         # counts = cap occur, unused slots too
            assert (b.counts[:, 1] == 4).any() and (b.counts[:, 1] < 4).any() and (b.counts[:, 3] == 2).any() and (b.counts[:, 3] < 2).any()


def test_check_instances_limits(drivers, tmp_path):
    def one(n_anchors=2, bw=2, caps=(5, 3, 2, 2)):
        b = Batch(1, *caps, bw, n_anchors=n_anchors)
        for _ in range(4):
            b.add_pose(0)
        return b
    cases = []

    def case(want, b, fill):
        fill(b)
        cases.append((want, b))
    case(0, one(), lambda b: (b.add_range(0, 0, 1), b.add_prior(0, 3), b.add_se3(0, 3, 2)))
    case(2, one(), lambda b: b.add_range(0, 4, 3))                       # index = nv
    case(2, one(), lambda b: b.add_range(0, 3, 4))
    case(2, one(), lambda b: b.add_range(0, -1, 0))
    case(4, one(), lambda b: b.add_prior(0, 4))
    case(4, one(), lambda b: b.add_prior(0, -1))
    case(5, one(), lambda b: b.add_se3(0, 4, 3))
    case(5, one(), lambda b: b.add_se3(0, 3, 4))
    case(5, one(), lambda b: b.add_se3(0, 0, -1))                        # an SE3 edge never names an anchor
    case(2, one(), lambda b: b.add_range(0, 0, -3))                      # -1 - n_anchors
    case(0, one(), lambda b: b.add_range(0, 0, -2))                      # -n_anchors: the last anchor
    case(2, one(n_anchors=0), lambda b: b.add_range(0, 0, -1))
    case(2, one(), lambda b: b.add_range(0, 2, 2))                       # self-edges
    case(5, one(), lambda b: b.add_se3(0, 2, 2))
    case(0, one(), lambda b: (b.add_range(0, 0, 2), b.add_range(0, 3, 1), b.add_se3(0, 1, 3), b.add_se3(0, 2, 0)))   # exactly bw_max
    case(3, one(), lambda b: b.add_range(0, 0, 3))                       # bw_max + 1
    case(3, one(), lambda b: b.add_range(0, 3, 0))
    case(6, one(), lambda b: b.add_se3(0, 0, 3))
    case(6, one(), lambda b: b.add_se3(0, 3, 0))
    case(0, one(bw=0), lambda b: b.add_range(0, 3, -1))                  # the distance rule is for pose-to-pose edges
    full = one()
    full.add_pose(0)
    for k in range(3):
        full.add_range(0, k, k + 1)
    for k in range(2):
        full.add_prior(0, 4); full.add_se3(0, k, k + 1)
    assert full.counts[0].tolist() == [5, 3, 2, 2]
    cases.append((0, full))                                              # counts = cap
    for k in range(4):
        for value, want in ((full.caps[k] + 1, 1), (-1, 1), (I32_MIN, 1), (I32_MAX, 1)):
            b = full.copy("counts")
            b.counts[0, k] = value
            cases.append((want, b))
    for want, b in cases:
        assert M.first_failed_check(b, 0) == want
    out = run(drivers, tmp_path, [b for _, b in cases])
    assert [int(o["check"][0]) for o in out] == [want for want, _ in cases]


def test_check_instances_two_faults_in_two_thread_ranges(drivers, tmp_path):
    n = 4096
    base = small_windows(n)
    both = corrupt(corrupt(base, 5, 2), n - 3, 5)
    one_range = corrupt(corrupt(base, 5, 6), 9, 4)                        # in ONE range the first instance decides
    out = run(drivers, tmp_path, [both, one_range], tsan=True)
    for key in ("check", "check_tsan"):
        assert int(out[0][key][0]) in (2, 5)
        if len(M.thread_ranges(n, drivers["hw"])) == 1:
            assert int(out[0][key][0]) == 2
        assert int(out[1][key][0]) == 6


# ---- chain_scan, translation_only -----------------------------------------------------------------------------------------------

def chain_window(rng, flavour, nv_max=7):
    """One window: an ordered chain, changed by `flavour`."""
    b = Batch(1, nv_max, 3 * nv_max, nv_max, 2 * nv_max, 3, n_anchors=2)
    nv = int(rng.integers(3, nv_max + 1))
    for k in range(nv):
        b.add_pose(0, rng.normal(size=3))
    edges = []
    for k in range(nv):
        if rng.random() < 0.5:
            edges.append((k, -1 - int(rng.integers(2))))
        if k and (rng.random() < 0.8 or k in (1, nv - 1)):
            edges.append((k - 1, k) if rng.random() < 0.5 else (k, k - 1))
    links = [e for e in edges if e[1] >= 0]
    se3 = []
    if flavour in ("se3", "second_se3", "second_both", "se3_out_of_order"):
        se3 = [((k - 1, k) if rng.random() < 0.5 else (k, k - 1)) for k in range(1, nv)]
    if flavour in ("second_range", "second_both"):
        at = edges.index(links[int(rng.integers(len(links)))])
        edges.insert(at + 1, edges[at][::-1] if rng.random() < 0.5 else edges[at])
    if flavour in ("second_se3", "second_both"):
        at = int(rng.integers(len(se3)))
        se3.insert(at, se3[at][::-1])
    if flavour == "out_of_order":                                         # one edge in front of an edge of an EARLIER pose
        at = int(rng.integers(1, len(edges)))
        while max(edges[at]) == max(edges[at - 1]):
            at = at % (len(edges) - 1) + 1
        edges[at - 1], edges[at] = edges[at], edges[at - 1]
    if flavour == "se3_out_of_order":
        se3[0], se3[-1] = se3[-1], se3[0]
    if flavour == "skip":
        edges.append((nv - 1, nv - 3))
    if flavour == "se3_skip":
        se3.append((0, 2))
    for e in edges:
        b.add_range(0, *e)
    for e in se3:
        b.add_se3(0, *e)
    pri = sorted(rng.integers(0, nv, int(rng.integers(4))).tolist())
    if flavour == "prior_out_of_order":
        pri = [nv - 1, 0]
    for v in pri:
        b.add_prior(0, v)
    return b


FLAVOURS = ("chain", "se3", "out_of_order", "se3_out_of_order", "prior_out_of_order", "second_range", "second_se3", "second_both", "skip", "se3_skip")


def assert_scans(b, o):
    got = [bool(x) for x in o["chain_scan"]]
    for k, ordered in enumerate((True, False)):
        chain, single, se3 = M.chain_scan(b, ordered)
        assert got[3 * k] == chain, (ordered, got)
        if M.chain_scan(b, True)[0]:          # the pair verdicts: chain batches in edge order, where every edge was scanned next to its twin
            assert got[3 * k + 1:3 * k + 3] == [single, se3], (ordered, got)
    assert bool(o["translation"][0]) == M.translation_only(b)
    assert int(o["envelope"][0]) == M.envelope_blocks_max(b)


def test_chain_scan_and_translation_only_match_the_model(drivers, tmp_path):
    rng = np.random.default_rng(11)
    batches, names = [], []
    for flavour in FLAVOURS:
        for _ in range(12):
            batches.append(chain_window(rng, flavour)); names.append(flavour)
    for seed in range(6):
        batches.append(small_windows(5 + seed, seed=100 + seed)); names.append("random")
        batches.append(small_windows(5 + seed, seed=200 + seed, chains=True)); names.append("random chains")
    verdicts = {}
    for name, b, o in zip(names, batches, run(drivers, tmp_path, batches)):
        assert int(o["check"][0]) == 0, name
        assert_scans(b, o)
        verdicts.setdefault(name, set()).add(tuple(int(x) for x in o["chain_scan"]))
    # the flavours do what their names say (ordered: chain, single_pairs, se3_pairs; any order: the same three)
    assert verdicts["chain"] == {(1, 1, 0, 1, 1, 0)} and verdicts["se3"] == {(1, 0, 1, 1, 0, 1)}
    assert verdicts["second_range"] == {(1, 0, 0, 1, 0, 0)} and verdicts["second_se3"] == {(1, 0, 0, 1, 0, 0)} and verdicts["second_both"] == {(1, 0, 0, 1, 0, 0)}
    for name in ("out_of_order", "se3_out_of_order", "prior_out_of_order"):
        assert {(v[0], v[3]) for v in verdicts[name]} == {(0, 1)}, name
    for name in ("skip", "se3_skip"):
        assert {(v[0], v[3]) for v in verdicts[name]} == {(0, 0)}, name


def test_translation_only_single_entries_flip_it(drivers, tmp_path):
    rng = np.random.default_rng(5)
    base = Batch(3, 5, 8, 3, 1, 4, n_anchors=2)
    for i in range(3):
        for k in range(4):
            base.add_pose(i, rng.normal(size=3))
        for k in range(1, 4):
            base.add_range(i, k - 1, k, 0.5, 2.0); base.add_range(i, k, -1, 3.0, 1.0)
        base.add_prior(i, 0, rng.normal(size=3)); base.add_prior(i, 3, rng.normal(size=3), info=(1.0, 2.0, 3.0, 0.0, 0.0, 0.0))
    batches = [base]

    def variant(table, index, value, **kw):
        b = base.copy(table)
        getattr(b, table)[index] = value
        for k, v in kw.items():
            setattr(b, k, v)
        batches.append(b)
    for k in range(9):
        variant("poses", (2, 3, k), 0.5)                                  # one rotation entry
    variant("poses", (0, 0, 0), -1.0)
    for k in (2, 3, 4):
        variant("r_val", (2, 5, k), 1e-300)                               # one lever-arm component
    for k in (15, 16, 17):
        variant("p_val", (2, 1, k), 1e-9)                                 # one rotation-information entry
    for k in range(9):
        variant("p_val", (1, 0, k), 0.25)                                 # a prior's measurement rotation
    se3 = base.copy("counts", "s_idx", "s_val")
    se3.add_se3(2, 0, 1)
    batches.append(se3)
    big = base.copy()
    big.n_anchors = 500001
    batches.append(big)
    n_flip = len(batches) - 1
    # what must NOT flip it: translations, measurements, prior translations and translation information, unused slots, 500 000 anchors
    variant("poses", (1, 2, 10), 7.0); variant("r_val", (1, 2, 0), 9.0); variant("r_val", (1, 2, 1), 9.0)
    variant("p_val", (1, 1, 10), 4.0); variant("p_val", (1, 1, 13), 4.0)
    variant("poses", (1, 4, 0), 3.0); variant("r_val", (0, 7, 3), 1.0); variant("p_val", (0, 2, 16), 1.0)
    ok = base.copy()
    ok.n_anchors = 500000
    batches.append(ok)
    out = run(drivers, tmp_path, batches)
    got = [int(o["translation"][0]) for o in out]
    assert got == [1] + [0] * n_flip + [1] * (len(batches) - 1 - n_flip)
    assert got == [int(M.translation_only(b)) for b in batches]


def test_scans_decided_by_the_last_instance_of_a_threaded_batch(drivers, tmp_path):
    n = 4100
    last = n - 1
    base = small_windows(n, chains=True).copy("counts", "r_idx", "r_val", "p_idx", "p_val")
    base.counts[last] = (3, 0, 0, 0)
    base.add_range(last, 0, 1); base.add_range(last, 2, 1)
    assert M.chain_scan(base, True) == (True, True, False) and M.translation_only(base)
    skip = base.copy("counts", "r_idx", "r_val").with_caps(bw_max=2)
    skip.add_range(last, 2, 0)
    twin = base.copy("counts", "r_idx", "r_val")
    twin.add_range(last, 1, 2)
    lever = base.copy("r_val")
    lever.r_val[last, 0, 4] = 0.25
    disorder = base.copy("counts", "p_idx", "p_val")
    disorder.add_prior(last, 1); disorder.add_prior(last, 0)
    batches = [base, skip, twin, lever, disorder]
    out = run(drivers, tmp_path, batches, tsan=True)
    for b, o in zip(batches, out):
        assert int(o["check"][0]) == 0 and int(o["check_tsan"][0]) == 0
        assert_scans(b, o)
    assert [tuple(int(x) for x in o["chain_scan"][[0, 3]]) for o in out] == [(1, 1), (0, 0), (1, 1), (1, 1), (0, 1)]
    assert [int(out[k]["chain_scan"][1]) for k in (0, 2, 3)] == [1, 0, 1]         # the twin of a pair, in the last window only
    assert [int(o["translation"][0]) for o in out] == [1, 1, 1, 0, 1]


# ---- hash_structure -------------------------------------------------------------------------------------------------------------

def test_hash_structure_sees_structure_and_nothing_else(drivers, tmp_path):
    base = small_windows(16, seed=3)
    batches = [base]
    same = 0
    for table, poison in (("poses", 1.5), ("r_val", 2.5), ("p_val", 3.5), ("s_val", 4.5)):            # values, used and unused
        b = base.copy(table); getattr(b, table)[...] = poison; batches.append(b); same += 1
    unused = base.copy("r_idx", "p_idx", "s_idx")
    for i in range(base.n):
        _, nr, npr, ns = base.counts[i]
        unused.r_idx[i, nr:] = 1; unused.p_idx[i, npr:] = 1; unused.s_idx[i, ns:] = 1
    batches.append(unused); same += 1
    for i in range(base.n):                                                                             # every used index, every count
        nv, nr, npr, ns = (int(x) for x in base.counts[i])
        entries = [("counts", (i, k)) for k in range(4)] + [("r_idx", (i, e, k)) for e in range(nr) for k in range(2)]
        entries += [("p_idx", (i, e)) for e in range(npr)] + [("s_idx", (i, e, k)) for e in range(ns) for k in range(4)]
        for table, index in entries:
            old = int(getattr(base, table)[index])
            values = [v for v in range(0, base.caps[index[1]] + 1) if v != old] if table == "counts" else [v for v in (-3, -2, -1, 0, 1, 2, 3, 4, old ^ 0x10000, old + (1 << 30)) if v != old]
            for v in values:
                b = base.copy(table); getattr(b, table)[index] = v; batches.append(b)
    assert len(batches) > 2000
    out = run(drivers, tmp_path, batches)
    h = [int(o["hash"][0]) for o in out]
    assert h[1:1 + same] == [h[0]] * same
    assert len(set(h[1 + same:] + [h[0]])) == len(h) - same, "two structures, one hash"
    assert all(int(o["hash"][1]) != int(o["hash"][0]) for o in out)                                    # has_off1
    assert len(set(int(o["hash"][1]) for o in out[1 + same:])) == len(h) - 1 - same


def test_hash_structure_threaded(drivers, tmp_path):
    n = 4099
    base = small_windows(n)
    batches = [base, base.copy("poses")]
    batches[1].poses[:, :, 9:] += 1.0
    for lo, hi in M.thread_ranges(n, drivers["hw"]):
        b = base.copy("p_idx"); b.p_idx[lo, 0] = (b.p_idx[lo, 0] + 1) % 3; batches.append(b)               # the first and the last window of the range
        b = base.copy("s_idx"); b.s_idx[hi - 1, int(base.counts[hi - 1, 3]) - 1, 2] ^= 1; batches.append(b)
    out = run(drivers, tmp_path, batches, tsan=True)
    h = [int(o["hash"][0]) for o in out]
    assert h[1] == h[0] and len(set(h[1:])) == len(h) - 1
    assert len(set(int(o["hash"][1]) for o in out[1:])) == len(h) - 1 and not set(h) & set(int(o["hash"][1]) for o in out)


# ---- envelope_blocks_max --------------------------------------------------------------------------------------------------------

def test_envelope_blocks_max(drivers, tmp_path):
    rng = np.random.default_rng(8)
    batches = []
    for _ in range(10):
        n = int(rng.integers(1, 6))
        b = Batch(n, 12, 20, 2, 6, 11, n_anchors=2)
        for i in range(n):
            nv = int(rng.integers(1, 13))
            for k in range(nv):
                b.add_pose(i)
            for _ in range(int(rng.integers(0, 21)) if nv > 1 else 0):
                v0 = int(rng.integers(nv))
                b.add_range(i, v0, -1 - int(rng.integers(2)) if rng.random() < 0.3 else int((v0 + rng.integers(1, nv)) % nv))
            for _ in range(int(rng.integers(0, 7)) if nv > 1 else 0):
                v0 = int(rng.integers(nv))
                b.add_se3(i, v0, int((v0 + rng.integers(1, nv)) % nv))
        batches.append(b)
    n_valid = len(batches)
    base = batches[0]
    assert base.counts[0, 1] >= 1 or base.counts[0, 3] >= 1
    for k in (0, 1, 3):                                                   # counts out of range (the priors are not this pass's business)
        for v in (base.caps[k] + 1, -1, I32_MAX, I32_MIN):
            b = base.copy("counts"); b.counts[base.n - 1, k] = v; batches.append(b)
    full = Batch(1, 4, 2, 1, 2, 3)
    for k in range(4):
        full.add_pose(0)
    full.add_range(0, 0, 1); full.add_range(0, 2, 3); full.add_se3(0, 1, 2); full.add_se3(0, 3, 0)
    batches.append(full)
    for table, index in (("r_idx", (0, 1, 0)), ("r_idx", (0, 1, 1)), ("s_idx", (0, 1, 0)), ("s_idx", (0, 1, 1))):
        for v in (4, I32_MAX, I32_MIN, -1):
            if table == "r_idx" and index[2] == 1 and v < 0:
                continue                                                   # (a range's second endpoint may be an anchor: any negative number here)
            b = full.copy(table); getattr(b, table)[index] = v; batches.append(b)
    out = run(drivers, tmp_path, batches)
    got = [int(o["envelope"][0]) for o in out]
    assert got == [M.envelope_blocks_max(b) for b in batches]
    assert all(g > 0 for g in got[:n_valid]) and got[n_valid:n_valid + 12] == [-1] * 12 and got[n_valid + 12] == 1 + 2 + 2 + 4 and got[n_valid + 13:] == [-1] * 14


# ---- build_tree_sched -----------------------------------------------------------------------------------------------------------

def forest_batch(rng, nv, n=3, shape="random"):
    pairs = []
    if shape == "path":
        order = rng.permutation(nv).tolist()
        pairs = list(zip(order[:-1], order[1:]))
    elif shape == "star":
        pairs = [(0, k) for k in range(1, nv)]
    else:
        order = rng.permutation(nv).tolist()
        for k in range(1, nv):
            if rng.random() < 0.8:                                        # else: a new component (maybe an isolated pose)
                pairs.append((order[int(rng.integers(max(0, k - 4) if shape == "deep" else 0, k))], order[k]))
    edges = []                                                            # ("r" | "s", v0, v1)
    for u, v in pairs:
        if rng.random() < 0.5:
            u, v = v, u
        kind = rng.random()
        if kind < 0.4 or kind > 0.8:
            edges.append(("r", u, v))
        if kind > 0.3:
            edges.append(("s", v, u) if rng.random() < 0.5 else ("s", u, v))
        if rng.random() < 0.2:
            edges.append(("r", v, u))                                     # a doubled edge on the pair
        if rng.random() < 0.1:
            edges.append(("s", u, v))
    for v in range(nv):
        for _ in range(int(rng.integers(0, 3))):
            edges.append(("r", v, -1 - int(rng.integers(3))))
    edges = [edges[k] for k in rng.permutation(len(edges))]
    priors = rng.integers(0, nv, int(rng.integers(0, 2 * nv))).tolist()
    nr, ns = sum(e[0] == "r" for e in edges), len(edges) - sum(e[0] == "r" for e in edges)
    b = Batch(n, nv + 1, nr + 2, len(priors) + 1, ns + 1, nv, n_anchors=3)
    for i in range(n):
        for k in range(nv):
            b.add_pose(i, rng.normal(size=3))
        for kind, u, v in edges:
            b.add_range(i, u, v, rng.random(), 1.0 + i) if kind == "r" else b.add_se3(i, u, v)
        for v in priors:
            b.add_prior(i, v, rng.normal(size=3))
    b.r_idx[1:, nr:] = 7; b.s_idx[1:, ns:] = 7                             # the windows differ in unused slots and in values only
    return b


def test_build_tree_sched_tables(drivers, tmp_path):
    rng = np.random.default_rng(21)
    batches = [forest_batch(rng, nv, shape=shape) for nv, shape in
               [(2, "path"), (2, "random"), (3, "star"), (64, "path"), (64, "star"), (64, "random"), (64, "deep"), (63, "deep")] +
               [(int(rng.integers(2, 65)), ("random", "deep")[k % 2]) for k in range(40)]]
    out = run(drivers, tmp_path, batches)
    seen_roots, seen_isolated = set(), False
    for b, o in zip(batches, out):
        assert int(o["check"][0]) == 0 and int(o["tree_ok"][0]) == 1
        M.check_tree_sched(b, o)
        seen_roots.add(int(o["tree_sizes"][5]))
        linked = set(b.r_idx[0, :b.counts[0, 1]][b.r_idx[0, :b.counts[0, 1], 1] >= 0].reshape(-1).tolist()) | set(b.s_idx[0, :b.counts[0, 3], :2].reshape(-1).tolist())
        seen_isolated = seen_isolated or len(linked) < int(b.counts[0, 0])
    assert len(seen_roots) > 3 and 1 in seen_roots and seen_isolated


def test_build_tree_sched_refusals(drivers, tmp_path):
    rng = np.random.default_rng(22)
    base = forest_batch(rng, 9)
    nv, nr, npr, ns = (int(x) for x in base.counts[0])
    assert nr >= 1 and npr >= 1 and ns >= 1
    refused, taken = [], [base]
    cyc = Batch(2, 6, 6, 1, 3, 5)
    for i in range(2):
        for k in range(5):
            cyc.add_pose(i)
        cyc.add_range(i, 0, 1); cyc.add_se3(i, 2, 1); cyc.add_range(i, 3, 4); cyc.add_range(i, 1, 0)
    taken.append(cyc.copy())
    cyc = cyc.copy("counts", "r_idx", "r_val")
    for i in range(2):
        cyc.add_range(i, 2, 0)                                            # 0 - 1 - 2 - 0
    refused.append(cyc)
    for nv1, ok in ((1, False), (2, True), (64, True), (65, False)):
        b = Batch(1, 65, 64, 1, 1, 64)
        for k in range(nv1):
            b.add_pose(0)
        for k in range(1, nv1):
            b.add_range(0, k, k - 1)
        (taken if ok else refused).append(b)
    off1 = base.copy(); off1.has_off1 = True
    refused.append(off1)
    last = base.n - 1
    for k in range(4):                                                    # the last window: one count (the slot it brings in holds a valid edge)
        b = base.copy("counts", "r_idx", "p_idx", "s_idx")
        b.r_idx[last, nr] = (0, -1); b.p_idx[last, npr] = 0; b.s_idx[last, ns] = (1, 0, 0, 0)
        b.counts[last, k] += 1
        refused.append(b)
    for table, index in [("r_idx", (last, nr - 1, 0)), ("r_idx", (last, 0, 1)), ("p_idx", (last, npr - 1)), ("s_idx", (last, ns - 1, 1)), ("s_idx", (last, 0, 0)), ("s_idx", (last, 0, 2))]:
        b = base.copy(table)                                              # one used index: another pose that is not the edge's other end
        t = getattr(b, table)
        taboo = {int(t[index])} | ({int(x) for x in t[index[:-1]][:2]} if table != "p_idx" else set())
        t[index] = 1 - t[index] if index[-1] == 2 and table == "s_idx" else next(v for v in range(nv) if v not in taboo)
        refused.append(b)
    for table, index, value in [("r_idx", (last, nr, 0), 0), ("p_idx", (last, npr), 0), ("s_idx", (last, ns, 1), 0), ("r_val", (last, 0, 0), 5.0), ("poses", (last, 0, 9), 5.0),
                                ("p_val", (last, 0, 9), 5.0), ("s_val", (last, 0, 9), 5.0)]:
        b = base.copy(table); getattr(b, table)[index] = value; taken.append(b)
    out = run(drivers, tmp_path, refused + taken)
    assert [int(o["check"][0]) for o in out] == [0] * len(out)
    assert [int(o["tree_ok"][0]) for o in out] == [0] * len(refused) + [1] * len(taken)
    for b, o in zip(taken, out[len(refused):]):
        M.check_tree_sched(b, o)
    assert all(M.is_forest(int(b.counts[0, 0]), [tuple(e) for e in b.r_idx[0, :b.counts[0, 1]].tolist() if e[1] >= 0] + [tuple(e[:2]) for e in b.s_idx[0, :b.counts[0, 3]].tolist()])
               for b in taken) and not M.is_forest(5, [(0, 1), (2, 1), (3, 4), (1, 0), (2, 0)])


def test_tree_and_arrow_builders_on_a_threaded_batch(drivers, tmp_path):
    """4 096 windows of one forest topology: the builders are single-threaded, but they run after the threaded passes on the same tables."""
    rng = np.random.default_rng(23)
    b = forest_batch(rng, 4, n=4096)
    o = run(drivers, tmp_path, [b], tsan=True)[0]
    assert int(o["check"][0]) == 0 == int(o["check_tsan"][0]) and int(o["tree_ok"][0]) == 1
    M.check_tree_sched(b, o)
    assert_scans(b, o)


# ---- build_arrow_aux ------------------------------------------------------------------------------------------------------------

def arrow_batch(rng, shapes, nv_max=None, n_anchors=4):
    """shapes: (chain poses n0, border poses nb0) per window."""
    n = len(shapes)
    nv_max = nv_max or max(a + c for a, c in shapes) + 1
    nr_max = max(a * (2 * c + 3) + c * c + 8 for a, c in shapes)
    b = Batch(n, nv_max, nr_max, 3 * nv_max, 1, nv_max, n_anchors=n_anchors)
    for i, (n0, nb0) in enumerate(shapes):
        nv = n0 + nb0
        for k in range(nv):
            b.add_pose(i, rng.normal(size=3))
        nseg = M.arrow_nseg(n0)
        cut = [k * n0 // nseg for k in range(1, nseg)]                    # near the cuts: a missing link on either side (windows 1, 4, ..)
        edges = [(0, n0)] if n0 > 1 else []                               # (the first border slot is in the border: a non-consecutive edge)
        for k in range(n0):
            missing = (i % 3 == 1 and any(k - 1 <= c <= k for c in cut)) or rng.random() < 0.05
            if k and not missing:
                edges.append((k - 1, k) if rng.random() < 0.5 else (k, k - 1))
            for a in range(nb0):
                if rng.random() < (0.5 if nb0 < 6 else 0.2) and not (k == n0 - 1 and a == 0):
                    e = (k, n0 + a) if rng.random() < 0.7 else (n0 + a, k)
                    edges.append(e)
                    if rng.random() < 0.15:
                        edges.append(e[::-1] if rng.random() < 0.5 else e)   # a doubled (pose, border) range
            if rng.random() < 0.3:
                edges.append((k, -1 - int(rng.integers(n_anchors))))
        for a in range(nb0):
            for c in range(a):
                if rng.random() < 0.4:
                    edges.append((n0 + a, n0 + c) if rng.random() < 0.5 else (n0 + c, n0 + a))
                    if rng.random() < 0.2:
                        edges.append((n0 + a, n0 + c))
            if rng.random() < 0.5:
                edges.append((n0 + a, -1 - int(rng.integers(n_anchors))))
        for c in cut:
            edges.append((c, -1))                                         # anchor ranges and priors on the poses next to and at the cuts
        order = rng.permutation(len(edges))
        for k in order:
            b.add_range(i, *edges[k], meas=float(rng.random()) + 0.5, info=float(rng.random()) + 1.0)
        for v in rng.integers(0, nv, nv // 2 + 2).tolist() + [c + d for c in cut for d in (-1, 0, 0, 1)] + [nv - 1, nv - 1, n0]:
            b.add_prior(i, int(v), rng.normal(size=3), info=tuple(rng.random(3) + 0.5) + (0.0, 0.0, 0.0))
    return b


def assert_arrow(b, o):
    assert int(o["check"][0]) == 0
    assert int(o["arrow"][0]) == 1 and int(o["arrow_only"][0]) == 1, [M.arrow_border(b, i) for i in range(b.n)]
    nb_max, jmax, jpmax, jch, jpch, list_cap = M.check_arrow_tables(b, o)
    assert o["arrow"][1:].tolist() == [list_cap, nb_max, jmax, jpmax] + jch + jpch
    assert int(o["arrow_only"][1]) == list_cap and o["arrow_only_len"].tolist() == [0, 0]      # structure_only: the verdict, the list size, nothing packed
    assert max(jch) <= jmax and max(jpch) <= jpmax


def test_build_arrow_aux_tables(drivers, tmp_path):
    rng = np.random.default_rng(31)
    n0s = [2, 23, 24, 47, 48, 71, 72, 95, 96, 131]
    batches = [arrow_batch(rng, [(n0, int(rng.integers(1, 13))) for n0 in n0s]),                       # ragged: every cut in one batch
               arrow_batch(rng, [(n0, nb0) for n0, nb0 in zip(n0s, (12, 1, 12, 1, 12, 1, 12, 1, 12, 1))]),
               arrow_batch(rng, [(n0, nb0) for n0, nb0 in zip(n0s, (1, 12, 1, 12, 1, 12, 1, 12, 1, 12))])]
    batches += [arrow_batch(rng, [(n0, int(rng.integers(1, 13)))]) for n0 in n0s]                       # and every cut on its own
    batches += [arrow_batch(rng, [(int(rng.integers(2, 140)), int(rng.integers(1, 13))) for _ in range(int(rng.integers(1, 6)))]) for _ in range(8)]
    out = run(drivers, tmp_path, batches)
    for b, o in zip(batches, out):
        assert_arrow(b, o)
    hdr = out[0]["ahdr"].reshape(-1, 8)
    assert hdr[:, 1].tolist() == [1, 1, 1, 1, 2, 2, 3, 3, 4, 4]


def test_build_arrow_aux_refusals(drivers, tmp_path):
    def window(n0, nb0, nv_max=None, n_anchors=300, extra=0, np_max=20):
        b = Batch(1, nv_max or n0 + nb0 + 1, n0 + nb0 + 70 + extra, np_max, 1, nv_max or n0 + nb0 + 1, n_anchors=n_anchors)
        for k in range(n0 + nb0):
            b.add_pose(0)
        for k in range(1, n0):
            b.add_range(0, k - 1, k)
        for a in range(nb0):
            b.add_range(0, 0, n0 + a)
        return b
    refused, taken = [], []
    taken.append(window(5, 1)); taken.append(window(5, 12)); taken.append(window(2, 3))
    refused.append(window(5, 0))                                           # a chain: no border
    refused.append(window(5, 13))
    # fewer than two chain poses: a border exists only through an edge between slots two or more apart, whose later end is slot 2 or
    # beyond, so slots 0 and 1 are always chain poses of a validated window; the nearest cases are these
    taken.append(window(1, 3))                                             # (0, 1) is a chain link: the border is the last two slots
    b = window(1, 2); b.counts[0, 1] = 0; b.add_range(0, 0, 2); taken.append(b)   # three poses, one edge: two chain poses without a link
    refused.append(window(1, 1))                                           # two poses joined by one edge: no border at all
    b = window(5, 2); b.add_range(0, 2, 1); refused.append(b)              # a second edge on a consecutive chain pair
    b = window(5, 2); b.add_range(0, 5, 6); b.add_range(0, 6, 5); taken.append(b)   # (on a border pair it is fine)
    b = window(5, 2); b.add_range(0, 3, -256); taken.append(b)             # anchor index 255
    b = window(5, 2); b.add_range(0, 3, -257); refused.append(b)           # anchor index 256
    for count, ok in ((63, True), (64, False)):                            # row 1 owns its link to row 0: 64 / 65 edges
        b = window(5, 2)
        for _ in range(count):
            b.add_range(0, 1, -1)
        (taken if ok else refused).append(b)
    for count, ok in ((16, True), (17, False)):
        b = window(5, 2)
        for _ in range(count):
            b.add_prior(0, 6)
        (taken if ok else refused).append(b)
    # the LDS limit: 96 chain poses (four segments) and a border of 12 make 15 border rows
    small, large = 528, 529
    assert M.arrow3_lds_bytes(small, 15) <= M.ARROW_LDS_LIMIT < M.arrow3_lds_bytes(large, 15) and M.arrow3_lds_bytes(large, 14) <= M.ARROW_LDS_LIMIT
    lds = window(96, 12, nv_max=large)
    taken.append(window(96, 12, nv_max=small))
    refused.append(lds)
    taken.append(window(96, 11, nv_max=large))
    out = run(drivers, tmp_path, refused + taken)
    assert [int(o["check"][0]) for o in out] == [0] * len(out)
    assert [(int(o["arrow"][0]), int(o["arrow_only"][0])) for o in out] == [(0, 0)] * len(refused) + [(1, 1)] * len(taken)
    for b, o in zip(taken, out[len(refused):]):
        assert_arrow(b, o)
