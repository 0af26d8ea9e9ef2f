"""Test helper: the inputs of the device-admitted resident slide (loc_window_slide_resident_dev; DESIGN.md §2, "The resident slide") that BOTH
tests/test_gpu_resident_slide_dev.py (the kernel's admission prologue) and tests/test_resident_slide_dev_cpu.py (slide_admit.h through its
stand-alone driver) run: one batch of eight windows of tests/_slide_ref.CASES["plain"] in which six windows are refused, each for another
rule, next to two regular ones — and the benign inputs of the same eight windows, which loc_window_slide_resident admits as a batch (the
yardstick of the regular windows).

Codes (include/localization_amd.h, LOC_SLIDE_ADMIT_*): 1 nv = 0; 2 a new count outside its range; 3 a new index outside rule 3; 4 / 5 / 6 the
slid window exceeds nv_max / nr_max / np_max; 7 a new row that is not translation-only."""
import numpy as np

import _fixed_lag as F
import _slide_ref as S

LOC_ERR_INVALID, LOC_ERR_UNSUPPORTED = -1, -5
NP_NEW_MAX = 4
REGULAR = (0, 7)
#          window:   0  1  2  3  4  5  6  7
CODES = {"a": [0, 2, 5, 4, 3, 6, 7, 0],    # count -1;            v0 = s - 2;                    a lever arm on a new range
         "b": [0, 2, 5, 4, 3, 6, 7, 0],    # count nr_new_max + 1; an anchor code >= n_anchors;   a rotated measurement of a new prior
         "c": [0, 1, 5, 4, 3, 6, 7, 0]}    # uploaded with nv = 0; a row on s - 1 after one on s; rotation information on a new prior


def status_of(codes):
    codes = np.asarray(codes)
    return np.where(codes == 0, 0, np.where(codes == 7, LOC_ERR_UNSUPPORTED, LOC_ERR_INVALID)).astype(np.int32)


def tight_batch(la):
    """(batch, chains, spec): the "plain" case under an nr_max that holds exactly its fullest window (window 2: five anchors per pose)"""
    wb, chains, spec = S.case_batch(la, "plain")
    full = int(np.argmax(wb.counts[:, 1]))
    assert full == 2
    small = la.WindowBatch(8, wb.caps[0], int(wb.counts[full, 1]), wb.caps[2], 0)
    small.counts[:] = wb.counts; small.poses[:] = wb.poses; small.p_idx[:] = wb.p_idx; small.p_val[:] = wb.p_val
    small.r_idx[:] = wb.r_idx[:, :small.caps[1]]; small.r_val[:] = wb.r_val[:, :small.caps[1]]
    return small, chains, spec


def _z_priors(chains, consumed, counts):
    pv = np.zeros((8, NP_NEW_MAX, 18)); pv[:, :, 0] = pv[:, :, 4] = pv[:, :, 8] = 1.0
    for i, ch in enumerate(chains):
        k = int(consumed[i])
        pv[i, :, 9:12] = -np.array([ch.est[k, 0], ch.est[k, 1], ch.truth[k, 2]])
        pv[i, :, 12:] = S.Z_INFO
    return np.asarray(counts, dtype=np.int32), pv


def benign_inputs(wb, chains, spec):
    """(new_pose, new_ranges, new_priors, drop_oldest) that loc_window_slide_resident admits for all eight windows: every window drops;
    window 7 appends one z prior.  Advances spec["consumed"]."""
    consumed = spec["consumed"].copy()
    pose, ranges, _, _ = S.next_inputs(wb, chains, spec)
    priors = _z_priors(chains, consumed, [0, 0, 0, 0, 0, 0, 0, 1])
    return pose, ranges, priors, np.ones(8, dtype=np.int32)


def refusing_inputs(wb, chains, spec, variant):
    """The same slide with windows 1 .. 6 breaking one rule each (CODES[variant]; variant "c" expects window 1 to have been uploaded
    EMPTY: empty_window() below).  spec["consumed"] as BEFORE benign_inputs() advanced it."""
    consumed = spec["consumed"]
    nv = wb.counts[:, 0].astype(int)
    drop = np.ones(8, dtype=np.int32)
    drop[3] = 0                                                     # 4: a full window that only grows (its rows name slot nv)
    slot = np.where(nv > 0, nv - drop, 0)
    pose, (rc, ri, rv) = S.new_rows(chains, consumed, slot, doubled=(2,))   # 5: a second link in the fullest window under a tight nr_max
    pc, pv = _z_priors(chains, consumed, [0, 0, 0, 0, 0, NP_NEW_MAX, 0, 1])  # 6: the carried prior and four new ones under np_max = 4
    s = int(slot[4])
    if variant == "a":
        rc[1] = -1
        ri[4, int(rc[4]) - 1] = (s - 2, s)
        rv[6, 0, 4] = 0.02
    elif variant == "b":
        rc[1] = ri.shape[1] + 1
        ri[4, 0] = (s, -1 - len(F.ANCH))
        pc[6] = 1; pv[6, 0, :9] = np.array([0, -1, 0, 1, 0, 0, 0, 0, 1.0])
    else:
        ri[4, 1] = (s - 1, -1)
        pc[6] = 1; pv[6, 0, 16] = 1e-300
    return pose, (rc, ri, rv), (pc, pv), drop


def empty_window(wb, i):
    """window i without poses (and so without rows): what variant "c" uploads as window 1"""
    wb.counts[i] = 0
    return wb
