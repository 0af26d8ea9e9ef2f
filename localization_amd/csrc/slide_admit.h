// The resident slide's per-window admission rule (loc_window_slide_resident_dev; DESIGN.md §2, "The resident slide"), stated once for the host
// and the device: plain C++ over ONE window's counts, its index tables and its new rows — no HIP types, no allocation, no library call.
// window_slide_kernel.hip's admission prologue restates it lane-parallel (rows over lanes, ballots for "any"); a host loop over this
// function is the CPU statement tests/host/slide_admit_driver.cpp holds to window_structure.cpp's slide_indices (the batch-wide rule of
// loc_window_slide_resident, with slide_rows_translation_only) window by window.
//
// The code of the FIRST check that fails, in this order (enum LOC_SLIDE_ADMIT_* of include/localization_amd.h):
//   1  the window has no pose (nv = 0)
//   2  a new count outside [0, nr_new_max] / [0, np_new_max]
//   3  a new range index outside rule 3: with s the new slot, v0 in {s - 1, s}; v1 in {s - 1, s} or an anchor code -1 - a, a in [0, n_anchors);
//      v0 != v1; a pose-to-pose row needs bw_max >= 1; no row on s - 1 alone after a row that names s
//   4 / 5 / 6  the slid window exceeds nv_max / nr_max / np_max (the carried prior's row counted iff a pose-to-pose range joins slot 0 to a pose)
//   7  a new row that is not translation-only: new_pose's rotation or a new prior's measurement rotation is not the identity's bit pattern,
//      a new range has a lever arm, a new prior has rotation information
// 0: admitted.  Rows beyond a count are never read; no row is read before both counts are known to be in range.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define LOCAMD_SLIDE_HD __host__ __device__
#else
#define LOCAMD_SLIDE_HD
#endif

namespace locamd {

enum SlideAdmit : int {
    kSlideAdmitOk = 0, kSlideAdmitNoPoses = 1, kSlideAdmitCount = 2, kSlideAdmitIndex = 3, kSlideAdmitNvMax = 4, kSlideAdmitNrMax = 5,
    kSlideAdmitNpMax = 6, kSlideAdmitNotTranslation = 7
};

// one window of the resident batch and what the call appends to it
struct SlideWindow {
    int nv_max, nr_max, np_max, bw_max;   // the handle's capacities
    int n_anchors;                        // the anchor table's size at call time
    int nv, nr, np;                       // the window's counts
    const int32_t* r_idx;                 // [nr][2]
    const int32_t* p_idx;                 // [np]
    bool drop;                            // the window drops slot 0
    int nr_new_max, nr_new;               // the call's capacity, this window's count
    const int32_t* new_r_idx;             // [nr_new_max][2]
    const double* new_r_val;              // [nr_new_max][5]
    int np_new_max, np_new;
    const double* new_p_val;              // [np_new_max][18]
    const double* new_pose;               // [12]
};

// the bit pattern of the 3 x 3 identity at v[0..8] (what std::memcmp with {1, 0, 0, 0, 1, 0, 0, 0, 1} tests: -0.0 is not 0.0 here)
LOCAMD_SLIDE_HD inline bool slide_identity_bits(const double* v) {
    bool same = true;
    for (int k = 0; k < 9; ++k) {
        unsigned long long bits;
        __builtin_memcpy(&bits, v + k, sizeof(bits));
        same = same && bits == (k % 4 == 0 ? 0x3FF0000000000000ull : 0ull);
    }
    return same;
}

LOCAMD_SLIDE_HD inline int slide_admit(const SlideWindow& w) {
    if (w.nv <= 0) return kSlideAdmitNoPoses;
    if (w.nr_new < 0 || w.nr_new > w.nr_new_max || w.np_new < 0 || w.np_new > w.np_new_max) return kSlideAdmitCount;
    const int sl = w.nv - (w.drop ? 1 : 0);   // the new slot: the slid window has sl + 1 poses
    bool named = false;                       // a row so far names the new slot
    for (int e = 0; e < w.nr_new; ++e) {
        const int32_t v0 = w.new_r_idx[e * 2], v1 = w.new_r_idx[e * 2 + 1];
        const bool ok0 = v0 == sl || (v0 == sl - 1 && v0 >= 0);
        const bool ok1 = v1 < 0 ? v1 >= -w.n_anchors : ((v1 == sl || v1 == sl - 1) && v1 != v0 && w.bw_max >= 1);
        const bool names = v0 == sl || v1 == sl;
        if (!ok0 || !ok1 || (named && !names)) return kSlideAdmitIndex;
        named = named || names;
    }
    // what the drop leaves: the kept rows, and whether a pose-to-pose range joined slot 0 to another pose (the marginal's slot >= 0)
    int r_kept = w.nr, p_kept = w.np, carried = 0;
    if (w.drop) {
        r_kept = 0; p_kept = 0;
        for (int e = 0; e < w.nr; ++e) {
            const int32_t v0 = w.r_idx[e * 2], v1 = w.r_idx[e * 2 + 1];
            if (v0 != 0 && v1 != 0) ++r_kept;
            else if (v1 >= 0) carried = 1;
        }
        for (int e = 0; e < w.np; ++e) p_kept += w.p_idx[e] != 0;
    }
    if (sl + 1 > w.nv_max) return kSlideAdmitNvMax;
    if (r_kept + w.nr_new > w.nr_max) return kSlideAdmitNrMax;
    if (carried + p_kept + w.np_new > w.np_max) return kSlideAdmitNpMax;
    if (!slide_identity_bits(w.new_pose)) return kSlideAdmitNotTranslation;
    for (int e = 0; e < w.nr_new; ++e) {
        const double* v = w.new_r_val + (size_t)e * 5;
        if (v[2] != 0.0 || v[3] != 0.0 || v[4] != 0.0) return kSlideAdmitNotTranslation;
    }
    for (int e = 0; e < w.np_new; ++e) {
        const double* v = w.new_p_val + (size_t)e * 18;
        if (!slide_identity_bits(v) || v[15] != 0.0 || v[16] != 0.0 || v[17] != 0.0) return kSlideAdmitNotTranslation;
    }
    return kSlideAdmitOk;
}

}  // namespace locamd
