"""The kernels that linearise the 6-DoF range, prior and EdgeSE3 factors, through localization_amd/csrc/se3_edge_device.h or on their own text,
compute, bit for bit, what their written-out copies computed: tests/golden/edge_terms_parent_bits.npz was recorded by
tools/record_edge_bits.py with the library of the commit before the factors were shared, and every case of that tool, run here on the built
library from the same seeded inputs, must give the same arrays (large arrays: the same digest of every window).  A difference in any bit is
a reordered operation, not a tolerance question."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_edge_bits as R  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden", "edge_terms_parent_bits.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_every_case_was_recorded(golden):
    """no case was left out of the recording (the tool leaves out a case whose two runs on the parent differ)"""
    recorded = {tuple(k.split("/")[:2]) for k in golden}
    assert recorded == set(R.case_ids()), set(R.case_ids()) ^ recorded


@pytest.mark.parametrize("name,jac", R.case_ids())
def test_same_bits_as_the_parent(gpu, golden, name, jac):
    import localization_amd as la
    got, kind = R.run_case(la, name, jac)
    want_kind = R.CASES[name][5]
    assert want_kind is None or kind == want_kind, (kind, want_kind)
    want = {k.split("/", 2)[2]: v for k, v in golden.items() if k.startswith(f"{name}/{jac}/")}
    assert want and got.keys() == want.keys(), (sorted(got), sorted(want))
    for k in sorted(got):
        same = np.array_equal(got[k], want[k])
        if not same and got[k].shape == want[k].shape:
            bad = np.flatnonzero(got[k].ravel() != want[k].ravel())
            print(f"{name}/{jac}/{k}: {bad.size} of {got[k].size} words differ, first at {bad[:8]}")
        assert same, f"{name}/{jac}/{k}"
