"""CPU checks of what WindowBatch states about itself (localization_amd/window.py): the table names, take / copy / tile, and the checks that
stand between a batch and the library's eight table pointers.  No device."""
import numpy as np
import pytest

import localization_amd as la
from localization_amd import _lib
from localization_amd.window import WindowBatch

CAPS = (4, 5, 2, 1)
EXTRAS = ("result", "p_info", "r_off1")


def _filled(B=3, caps=CAPS, extras=True):
    """every table (and result, p_info, r_off1) filled with values that differ everywhere"""
    wb = WindowBatch(B, *caps)
    if extras:
        wb.p_info = np.zeros((B, max(caps[2], 1), 36))
        wb.r_off1 = np.zeros((B, max(caps[1], 1), 3))
    start = 1
    for name in WindowBatch.TABLES + EXTRAS:
        a = getattr(wb, name)
        if a is not None:
            a[...] = np.arange(start, start + a.size).reshape(a.shape)
            start += a.size
    return wb


def test_tables_are_the_abi_argument_order():
    assert WindowBatch.TABLES == ("counts", "poses", "r_idx", "r_val", "p_idx", "p_val", "s_idx", "s_val")
    assert la.WindowBatch is WindowBatch


def test_take_copies_the_named_rows_of_everything():
    wb = _filled()
    before = {n: getattr(wb, n).copy() for n in WindowBatch.TABLES + EXTRAS}
    rows = [2, 0, 2, 1]
    out = wb.take(rows)
    assert out.B == 4 and out.caps == wb.caps
    for name in WindowBatch.TABLES + EXTRAS:
        got, src = getattr(out, name), getattr(wb, name)
        assert got.dtype == src.dtype and got.shape == (4,) + src.shape[1:], name
        assert np.array_equal(got, src[rows]), name
        assert got.flags.c_contiguous and got.flags.owndata and not np.shares_memory(got, src), name
        got[...] = 0
        assert np.array_equal(src, before[name]), name
    same = wb.copy()
    assert same.B == wb.B and all(np.array_equal(getattr(same, n), before[n]) for n in WindowBatch.TABLES + EXTRAS)


def test_none_stays_none():
    out = _filled(extras=False).take([2, 0, 2, 1])
    assert out.p_info is None and out.r_off1 is None
    assert _filled(extras=False).copy().p_info is None and _filled(extras=False).tile(7).r_off1 is None


def test_tile_is_the_three_old_spellings():
    wb = _filled()
    out = wb.tile(7)
    assert out.B == 7
    for name in WindowBatch.TABLES + EXTRAS:
        src = getattr(wb, name)
        assert np.array_equal(getattr(out, name), np.resize(src, (7,) + src.shape[1:])), name
        assert np.array_equal(getattr(out, name), np.concatenate([src] * 3)[:7]), name
        assert np.array_equal(getattr(out, name), src[np.arange(7) % wb.B]), name
    short = wb.tile(2)
    assert short.B == 2 and all(np.array_equal(getattr(short, n), getattr(wb, n)[:2]) for n in WindowBatch.TABLES + EXTRAS)


def test_a_capacity_of_zero_copies_and_tiles():
    wb = _filled(caps=(4, 5, 0, 0), extras=False)
    assert wb.p_idx.shape == (3, 1) and wb.s_val.shape == (3, 1, 48)
    for out, rows in ((wb.copy(), np.arange(3)), (wb.tile(7), np.arange(7) % 3)):
        assert out.caps == (4, 5, 0, 0) and len(out._pointers()) == 8
        for name in WindowBatch.TABLES:
            assert np.array_equal(getattr(out, name), getattr(wb, name)[rows]), name


def test_the_pointers_come_in_tables_order_after_the_checks():
    wb = _filled()
    ptrs = wb._pointers()
    assert len(ptrs) == 8
    for name, p in zip(WindowBatch.TABLES, ptrs):
        a = getattr(wb, name)
        assert p[0] == a.reshape(-1)[0] and type(p[0]) is (int if a.dtype == np.int32 else float), name


def _sliced(wb):
    big = np.zeros((wb.B, 2 * wb.caps[1], 5))
    wb.r_val = big[:, ::2]
    assert wb.r_val.shape == (wb.B, wb.caps[1], 5) and not wb.r_val.flags.c_contiguous


def _float32_poses(wb):
    wb.poses = wb.poses.astype(np.float32)


def _int64_counts(wb):
    wb.counts = wb.counts.astype(np.int64)


def _short(wb):
    wb.s_idx = np.ascontiguousarray(wb.s_idx[:2])


@pytest.mark.parametrize("spoil, table", [(_sliced, "r_val"), (_float32_poses, "poses"), (_int64_counts, "counts"), (_short, "s_idx")])
def test_a_table_the_library_would_misread_is_refused_by_name(spoil, table):
    wb = _filled()
    spoil(wb)
    with pytest.raises(ValueError, match=rf"\b{table}\b"):
        wb._pointers()
    with pytest.raises(ValueError, match=rf"\b{table}\b"):   # (the plan calls are host only: the check stands before them too)
        la.window.covariance_plan(wb)


def test_every_window_entry_has_argtypes(built):
    L = la.lib()
    names = [n for n in _lib.EXPORTED_SYMBOLS if n.startswith("loc_window_")]
    assert len(names) > 40
    for n in names:
        assert getattr(L, n).argtypes is not None, n
