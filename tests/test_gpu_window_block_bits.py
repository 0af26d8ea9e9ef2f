"""window_lm_kernel computes, bit for bit, what it computed at the commit this guard was added in: tests/golden/window_block_steps_parent_bits.npz
was recorded by tools/record_window_block_bits.py with that commit's parent library, and every case of that tool, run here on the built library,
must give the same 64-bit digest for every window (solved poses and result row).  A difference in any bit is a reordered operation, not a
tolerance question.  The guard is for the 6x6 block steps of factor_and_solve_sparse and factor_and_solve_small: the ones that call
localization_amd/csrc/window_block_device.h and the ones kept as written-out copies of its functions alike — whoever turns a
copy into a call, or touches one, learns here whether the bits stayed.

Which case reaches which of those sites (tests/_elimination_model.py gives the C / R / W mode of every level; C and W levels are column mode):
  column mode without pushed columns   arrays in LDS, records too many for the small schedule: lds3 clique12 (its last two levels);
  column mode with pushed columns      ws6 tree40 (39 of 40 columns pushed, every level C), chain30clique8 (23), pad5, fallback6 chain30; the wide
                                       first level (W) of grid8x8 in ws6 / ws3: 24 columns with off-diagonal blocks, none pushed; eight-word masks:
                                       wide6 / wide3 components130 in the caller's order (65 pushed), pendant (its first level), dense6 / dense3;
    B B^T and B y taken off (G, y)     every window whose last levels are "CC" (ring, grid, clique, ladder: the last column's row holds an unpushed block);
    block x block^T into the block     the same windows (block (last, last - 1) has earlier columns in common);
  row mode, kinds 0 / 1 / 2            every R level: diagonal rows, rows of off-diagonal blocks (every batch but the pure trees and chains has
                                       them), right-hand sides — one-word masks in LDS (lds3 clique12), in the workspace (ws6, ws3, fallback6:
                                       its first window in the caller's order, the fallback), eight-word masks (wide6, wide3, dense6, dense3, selfcal6);
  the small schedule's stage B         lds6 (all four windows) and lds3 clique10, ring12, components14, and its back-substitution;
  the level-by-level back-substitution every window of the other batches but sky6 (the SKYLINE sweep: its text is the parent's);
  a failed factorisation after steps   "third negated" — lds6 (stage B's inverse-pivot test), ws6 (column and row mode, one-word masks), wide6
                                       (eight-word masks) — and "root" (selfcal6: the root supernode): terminated = 1 or extra trials in the result row."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_window_block_bits as R  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden", "window_block_steps_parent_bits.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_every_case_was_recorded(golden):
    """no case was left out of the recording (the tool leaves out a case whose two runs on the parent differ)"""
    assert set(golden) == {R.key(c) for c in R.case_ids()}, set(golden) ^ {R.key(c) for c in R.case_ids()}


def test_the_failed_factorisations_fail(gpu):
    """the "third negated" inputs end windows on refused factorisations after accepted steps (terminated = 1 with outer > 1), on every schedule"""
    import localization_amd as la
    for name in R.THIRD_NEGATED:
        _, res, _ = R.run_case(la, "third negated", name, "analytic", "as built")
        assert np.isfinite(res).all() and ((res[:, 5] == 1) & (res[:, 3] > 1)).any(), (name, res[:, 3:6])


@pytest.mark.parametrize("case", R.case_ids(), ids=R.key)
def test_same_bits_as_the_parent(gpu, golden, case):
    import localization_amd as la
    got, res, kind = R.run_case(la, *case)
    assert kind == "window_lm_kernel", kind
    want = golden[R.key(case)]
    bad = np.flatnonzero(got != want) if got.shape == want.shape else None
    print(f"{R.key(case)}: outer {res[:, 3].astype(int).tolist()} trials {res[:, 4].astype(int).tolist()} terminated {res[:, 5].astype(int).tolist()}; windows that differ: {bad}")
    assert np.array_equal(got, want), (R.key(case), bad)
