"""§8(f) "next" rows on the CPU: the bag reader in front of the path, the ATE evaluation behind it, and the C++ shim header.
No solver runs here (the product has no CPU path)."""
import os
import subprocess

import numpy as np
import pytest

from localization_amd import ate, bag

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def ref_bag(tmp_path_factory):
    """The reference's recording bag/data_example.bag, stored xz-compressed as tests/golden/data_example.bag.xz."""
    import lzma
    path = tmp_path_factory.mktemp("bag") / "data_example.bag"
    with lzma.open(os.path.join(GOLD, "data_example.bag.xz")) as f:
        path.write_bytes(f.read())
    return str(path)


def test_associate_and_horn_alignment_known_answers():
    ta = np.arange(0, 10, 0.1)
    tb = ta + 0.004                       # inside the 20 ms window
    pairs = ate.associate(ta, tb)
    assert pairs == [(i, i) for i in range(len(ta))]
    assert ate.associate(ta, ta + 0.05) == []                    # 50 ms from every stamp: nothing within max_difference
    assert ate.associate([0.0, 1.0], [0.001, 0.002]) == [(0, 0)]  # one-to-one, best first
    rng = np.random.default_rng(0)
    P = rng.normal(size=(3, 200))
    th = 0.7
    R = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]])
    t = np.array([[1.0], [-2.0], [0.5]])
    Q = R @ P + t
    R2, t2, err = ate.horn_align(P, Q)
    assert np.allclose(R2, R, atol=1e-12) and np.allclose(t2, t, atol=1e-12) and err.max() < 1e-12
    est = np.column_stack([ta, P[:, :100].T]); tru = np.column_stack([tb, (R @ P[:, :100] + t).T])
    r = ate.evaluate_ate(est, tru)
    assert r["pairs"] == 100 and r["rmse"] < 1e-12
    r2 = ate.evaluate_ate(est, tru, align=False)
    assert r2["rmse"] > 1.0


def test_tum_round_trip(tmp_path):
    p = np.array([[1491129341.123456789, 0.1, -0.2, 1.1, 0.0, 0.0, 0.3826834, 0.9238795]])
    f = tmp_path / "traj.txt"
    ate.write_tum(str(f), p)
    ate.write_tum(str(f), p + 1)
    back = ate.read_tum(str(f))
    assert back.shape == (2, 8) and abs(back[0, 0] - p[0, 0]) < 1e-6 and np.allclose(back[0, 1:], p[0, 1:], atol=1e-6)


def test_ate_of_vicon_against_itself_and_fixture_sanity():
    z = np.load(os.path.join(GOLD, "bag_example.npz"))
    truth = np.column_stack([z["vicon_stamp"], z["vicon_pos"], z["vicon_q_xyzw"]])
    r = ate.evaluate_ate(truth[::2], truth)
    assert r["rmse"] < 1e-12 and r["pairs"] == len(truth[::2])
    noisy = truth.copy(); noisy[:, 1:4] += np.random.default_rng(1).normal(0, 0.05, (len(truth), 3))
    r = ate.evaluate_ate(noisy, truth)
    assert 0.07 < r["rmse"] < 0.1                                # sqrt(3) * 0.05


def test_native_ate_tool_matches_the_numpy_evaluation(tmp_path):
    """tools/loc_ate.cpp ("small native tool") on TUM files written by the node's log writer: the same association,
    alignment and statistics as localization_amd/ate.py — on the example recording's Vicon track against a rotated, shifted, noisy,
    time-offset and sub-sampled copy of it, aligned and not, and its error exit when no stamps match."""
    import json
    import shutil
    import subprocess
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "loc_ate")
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tools", "loc_ate.cpp"), "-o", exe])
    z = np.load(os.path.join(GOLD, "bag_example.npz"))
    truth = np.column_stack([z["vicon_stamp"], z["vicon_pos"], z["vicon_q_xyzw"]])
    rng = np.random.default_rng(4)
    from scipy.spatial.transform import Rotation
    Rm = Rotation.from_rotvec([0.2, -0.4, 1.1]).as_matrix()
    est = truth[::3].copy()
    est[:, 1:4] = est[:, 1:4] @ Rm.T + np.array([0.5, -2.0, 0.3]) + rng.normal(0, 0.03, (len(est), 3))
    est[:, 0] += 0.004 + rng.uniform(-0.003, 0.003, len(est))
    ft, fe = str(tmp_path / "truth.txt"), str(tmp_path / "est.txt")
    ate.write_tum(ft, truth, header=["truth"]); ate.write_tum(fe, est, header=["estimate"])
    t2, e2 = ate.read_tum(ft), ate.read_tum(fe)          # (what the files hold: '%g' keeps six digits of the coordinates)
    for extra, kw in (([], {}), (["--no-align"], {"align": False}), (["--offset", "-0.004", "--max_difference", "0.01"], {"offset": -0.004, "max_difference": 0.01})):
        got = json.loads(subprocess.check_output([exe, ft, fe] + extra))
        want = ate.evaluate_ate(e2, t2, **kw)
        assert got["pairs"] == want["pairs"] > 600
        for k in ("rmse", "mean", "median", "std", "min", "max"):
            assert abs(got[k] - want[k]) < 1e-9 * max(1.0, abs(want[k])), (extra, k, got[k], want[k])
    far = est.copy(); far[:, 0] += 100.0
    ate.write_tum(fe, far, header=["estimate"])
    r = subprocess.run([exe, ft, fe], capture_output=True, text=True)
    assert r.returncode == 1 and "matching timestamp pairs" in r.stderr


def test_bag_reader_reproduces_the_committed_fixture(ref_bag):
    z = np.load(os.path.join(GOLD, "bag_example.npz"))
    conns, msgs = bag.read_bag(ref_bag)
    types = {c.topic: c.msg_type for c in conns.values()}
    assert types["/uwb_endorange_info"] == "uwb_driver/UwbRange" and types["/imu/data"] == "sensor_msgs/Imu"
    assert [c.md5sum for c in conns.values() if c.msg_type == "uwb_driver/UwbRange"] == ["1b3efd633e416bfcfbaaf891dd23ac23"]
    ev = list(bag.events(ref_bag))
    rng = [e for e in ev if e["kind"] == "range"]; imu = [e for e in ev if e["kind"] == "imu"]; tru = [e for e in ev if e["kind"] == "truth"]
    assert (len(rng), len(imu), len(tru)) == (1444, 4514, 1965)
    assert np.array_equal(np.array([e["distance"] for e in rng], dtype=np.float32), z["uwb_distance"][np.argsort(z["uwb_rectime"], kind="stable")])
    assert all(a["record_time"] <= b["record_time"] for a, b in zip(ev, ev[1:]))
    assert rng[0]["frame_id"] == "uwb" and imu[0]["frame_id"] == "imu_link" and rng[0]["antenna"] == 1


def test_bz2_chunks_are_read(tmp_path):
    """Synthesise a one-chunk bag with a bz2-compressed chunk holding one connection and one Imu message."""
    import bz2
    import struct

    def rec(hdr, data):
        h = b"".join(struct.pack("<I", len(k) + 1 + len(v)) + k + b"=" + v for k, v in hdr.items())
        return struct.pack("<I", len(h)) + h + struct.pack("<I", len(data)) + data

    conn_data = b"".join(struct.pack("<I", len(k) + 1 + len(v)) + k + b"=" + v for k, v in
                         {b"topic": b"/imu/data", b"type": b"sensor_msgs/Imu", b"md5sum": b"x", b"message_definition": b"Header header"}.items())
    msg = struct.pack("<III", 7, 100, 500000000) + struct.pack("<I", 8) + b"imu_link" + struct.pack("<4d", 0, 0, 0, 1) + struct.pack("<9d", *([1e-6] * 9)) + bytes(8 * 24)
    inner = rec({b"op": b"\x07", b"conn": struct.pack("<I", 0), b"topic": b"/imu/data"}, conn_data) + \
        rec({b"op": b"\x02", b"conn": struct.pack("<I", 0), b"time": struct.pack("<II", 100, 600000000)}, msg)
    chunk = rec({b"op": b"\x05", b"compression": b"bz2", b"size": struct.pack("<I", len(inner))}, bz2.compress(inner))
    path = tmp_path / "one.bag"
    path.write_bytes(b"#ROSBAG V2.0\n" + rec({b"op": b"\x03", b"index_pos": struct.pack("<Q", 0), b"conn_count": struct.pack("<I", 1),
                                              b"chunk_count": struct.pack("<I", 1)}, bytes(16)) + chunk)
    ev = list(bag.events(str(path)))
    assert len(ev) == 1 and ev[0]["kind"] == "imu" and ev[0]["stamp"] == 100.5 and ev[0]["q_xyzw"] == (0, 0, 0, 1)
    assert ev[0]["record_time"] == pytest.approx(100.6)


def test_lz4_frame_decoder():
    """Known-answer blocks written by hand from the LZ4 block format, then whole frames from pyarrow's LZ4-frame codec
    (an independent encoder that is in the image) over compressible, incompressible and multi-block inputs."""
    from localization_amd import lz4frame
    out = bytearray()
    lz4frame.decode_block(bytes([0x50]) + b"hello", out)                        # literals only
    assert bytes(out) == b"hello"
    out = bytearray()
    lz4frame.decode_block(bytes([0x1F, 0x61, 0x01, 0x00, 0x05, 0x10, 0x62]), out)  # 'a', overlapping match len 4+15+5, then 'b'
    assert bytes(out) == b"a" * 25 + b"b"
    out = bytearray()
    lz4frame.decode_block(bytes([0x42]) + b"abcd" + bytes([0x02, 0x00, 0x10]) + b"!", out)  # offset 2 < match length 6
    assert bytes(out) == b"abcd" + b"cdcdcd" + b"!"
    with pytest.raises(ValueError):
        lz4frame.decode_block(bytes([0x10, 0x61, 0x05, 0x00]), bytearray())     # offset beyond the window
    pa = pytest.importorskip("pyarrow")
    rng = np.random.default_rng(0)
    for raw in (b"", b"x", b"abcabcabc" * 1000, rng.integers(0, 256, 70000, dtype=np.uint8).tobytes(),
                (b"range" + bytes(rng.integers(0, 4, 300, dtype=np.uint8))) * 20000):   # 6 MB: several 4 MB-max blocks
        comp = pa.compress(raw, codec="lz4", asbytes=True)
        assert lz4frame.decompress(comp, len(raw)) == raw
    with pytest.raises(ValueError):
        lz4frame.decompress(pa.compress(b"abc" * 100, codec="lz4", asbytes=True)[:-6], 300)
    with pytest.raises(ValueError):
        lz4frame.decompress(b"\x00" * 16)
    good = bytearray(pa.compress(b"abcabcabc" * 1000, codec="lz4", asbytes=True))
    for cut in range(8, len(good) - 1, 3):      # every truncation is reported as ValueError, never an IndexError or a hang
        with pytest.raises(ValueError):
            lz4frame.decompress(bytes(good[:cut]), 9000)


def test_lz4_chunks_are_read(tmp_path, ref_bag):
    """The reference bag re-chunked with compression=lz4 (chunks re-encoded here with pyarrow's LZ4-frame codec) decodes
    to the same event stream as the original."""
    pa = pytest.importorskip("pyarrow")
    import struct
    buf = open(ref_bag, "rb").read()
    out = bytearray(buf[:13])
    pos = 13
    n_chunks = 0
    while pos < len(buf):
        (hlen,) = struct.unpack_from("<I", buf, pos)
        hdr = buf[pos + 4:pos + 4 + hlen]
        (dlen,) = struct.unpack_from("<I", buf, pos + 4 + hlen)
        data = buf[pos + 8 + hlen:pos + 8 + hlen + dlen]
        if b"op=\x05" in hdr and b"compression=none" in hdr:
            hdr = hdr.replace(struct.pack("<I", 16) + b"compression=none", struct.pack("<I", 15) + b"compression=lz4")
            data = pa.compress(data, codec="lz4", asbytes=True)
            n_chunks += 1
        out += struct.pack("<I", len(hdr)) + hdr + struct.pack("<I", len(data)) + data
        pos += 8 + hlen + dlen
    assert n_chunks == 3
    path = tmp_path / "lz4.bag"
    path.write_bytes(bytes(out))
    a, b = list(bag.events(ref_bag)), list(bag.events(str(path)))
    assert len(a) == len(b) and a == b


@pytest.mark.parametrize("compression", ["none", "bz2", "lz4"])
def test_written_bag_round_trips_through_the_reader(tmp_path, compression):
    """The fixture re-serialised as a rosbag (tests/_bagwriter.py) and read back: every field the path uses survives,
    in record-time order, for each chunk compression the reader supports (no reference file needed: runs anywhere)."""
    if compression == "lz4":
        pytest.importorskip("pyarrow")
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from _bagwriter import write_bag
    z = np.load(os.path.join(GOLD, "bag_example.npz"))
    n = 200
    path = str(tmp_path / f"{compression}.bag")
    total = write_bag(path, z, n_ranges=n, compression=compression)
    ev = list(bag.events(path))
    assert len(ev) == total
    rng = [e for e in ev if e["kind"] == "range"]
    order = np.argsort(z["uwb_rectime"][:n], kind="stable")
    assert np.array_equal(np.array([e["distance"] for e in rng], dtype=np.float32), z["uwb_distance"][:n][order])
    assert np.array_equal(np.array([e["distance_err"] for e in rng], dtype=np.float32), z["uwb_distance_err"][:n][order])
    assert [e["responder_id"] for e in rng] == [int(v) for v in z["uwb_responder"][:n][order]]
    assert np.allclose([e["stamp"] for e in rng], z["uwb_stamp"][:n][order], atol=2e-9, rtol=0)
    imu = [e for e in ev if e["kind"] == "imu"]
    assert np.allclose(np.array([e["q_xyzw"] for e in imu]), z["imu_q_xyzw"][:len(imu)])
    tru = [e for e in ev if e["kind"] == "truth"]
    assert len(tru) > 100 and np.allclose(np.array([e["pose"][:3] for e in tru]), z["vicon_pos"][:len(tru)])
    assert all(a["record_time"] <= b["record_time"] for a, b in zip(ev, ev[1:]))


def test_associate_matches_the_reference_rule_on_dense_stamps():
    """script/associate.py:86-97 restated by brute force (all pairs inside max_difference, sorted by (difference, a, b),
    greedy): with stamps denser than max_difference a stamp whose two nearest partners are taken still gets the third."""
    from localization_amd import ate
    rng = np.random.default_rng(2)
    for trial in range(20):
        a = np.sort(rng.uniform(0, 1.0, 60)); b = np.sort(rng.uniform(0, 1.0, 80))
        md, off = 0.02, 0.003 * trial
        pot = sorted((abs(x - (y + off)), x, y) for x in a for y in b if abs(x - (y + off)) < md)
        fa, fb, want = set(a), set(b), []
        for _, x, y in pot:
            if x in fa and y in fb:
                fa.remove(x); fb.remove(y); want.append((x, y))
        want.sort()
        got = [(a[i], b[j]) for i, j in ate.associate(a, b, off, md)]
        assert got == want
    # the case the two-nearest shortcut dropped: b's nearest two taken by closer a's, a third still inside the window
    a = np.array([0.000, 0.004, 0.012]); b = np.array([0.001, 0.005, 0.030])
    assert ate.associate(a, b, 0.0, 0.02) == [(0, 0), (1, 1), (2, 2)]


def test_shim_header_compiles_standalone(tmp_path):
    src = tmp_path / "shim_use.cpp"
    src.write_text('#include "localization_amd_shim.hpp"\n'
                   "int use(localization_amd::Localization& l) {\n"
                   '  bool s = l.addRangeEdge(200, 100, 1.0, 3.0f, 0.055f, 1, "uwb");\n'
                   '  s |= l.addImuEdge(1.0, {{0, 0, 0, 1}}, {{1e-6, 0, 0, 0, 1e-6, 0, 0, 0, 1e-6}}, "imu_link");\n'
                   "  return (int)s + (int)l.optimizedPath().size() + (int)l.published();\n}\n")
    subprocess.check_call(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)])
