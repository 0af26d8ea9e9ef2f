// The per-window admission rule of the resident PLAIN-DROP slide of 6-DoF chain windows (loc_window_slide_plain_resident_dev; DESIGN.md §2,
// "The plain drop for 6-DoF chain windows"), stated once for the host and the device in slide_admit.h's way: plain C++ over ONE window's counts,
// its index tables and the index half of its new rows — no HIP types, no allocation, no library call.  window_slide_plain_kernel.hip's
// prologue restates it lane-parallel (rows over lanes, ballots for "any"); tests/host/slide_plain_admit_driver.cpp holds this function to a
// numpy statement of the rule.
//
// The code of the FIRST check that fails, in this order (enum LOC_SLIDE_ADMIT_* of include/localization_amd.h):
//   1  the window has no pose (nv = 0)
//   2  a new count outside [0, nr_new_max] / [0, np_new_max] / [0, ns_new_max]
//   3  a new index: a range row outside rule 3 of slide_admit.h (with s the new slot, v0 in {s - 1, s}; v1 in {s - 1, s} or an anchor code
//      -1 - a, a in [0, n_anchors); v0 != v1; a pose-to-pose row needs bw_max >= 1; no row on s - 1 alone after a row that names s), or an
//      EdgeSE3 row whose {vi, vj} is not {s - 1, s} (either order; needs s - 1 >= 0 and bw_max >= 1)
//   4 / 5 / 6 / 8  the slid window exceeds nv_max / nr_max / np_max / ns_max (nothing is carried: the kept rows plus the new ones)
//   9  the new rows break the pair rule the resident verdict was taken under — kSlidePairsWave6: any EdgeSE3 row, or more than one
//      pose-to-pose range row; kSlidePairsWave6S: more than one EdgeSE3 row, or more than one pose-to-pose range row; kSlidePairsNone: never
// 0: admitted.  Code 7 (a row that is not translation-only) does not exist here: no value is read at all.  Rows beyond a count are never
// read; no row is read before all three new counts are known to be in range.
#pragma once
#include <cstddef>
#include <cstdint>

#include "slide_admit.h"

namespace locamd {

enum SlidePlainAdmit : int { kSlideAdmitNsMax = 8, kSlideAdmitPairs = 9 };
// the pair rule of the resident verdict: LOC_WINDOW_KERNEL_CHAIN, _WAVE6 (single_pairs), _WAVE6S (se3_pairs)
enum SlidePairRule : int { kSlidePairsNone = 0, kSlidePairsWave6 = 1, kSlidePairsWave6S = 2 };

// one window of the resident batch and the index half of what the call appends to it
struct SlidePlainWindow {
    int nv_max, nr_max, np_max, ns_max, bw_max;   // the handle's capacities
    int n_anchors;                                // the anchor table's size at call time
    int pair_rule;                                // SlidePairRule
    int nv, nr, np, ns;                           // the window's counts
    const int32_t* r_idx;                         // [nr][2]
    const int32_t* p_idx;                         // [np]
    const int32_t* s_idx;                         // [ns][4]
    bool drop;                                    // the window drops slot 0
    int nr_new_max, nr_new;                       // the call's capacity, this window's count
    const int32_t* new_r_idx;                     // [nr_new_max][2]
    int np_new_max, np_new;
    int ns_new_max, ns_new;
    const int32_t* new_s_idx;                     // [ns_new_max][4]
};

LOCAMD_SLIDE_HD inline int slide_plain_admit(const SlidePlainWindow& w) {
    if (w.nv <= 0) return kSlideAdmitNoPoses;
    if (w.nr_new < 0 || w.nr_new > w.nr_new_max || w.np_new < 0 || w.np_new > w.np_new_max || w.ns_new < 0 || w.ns_new > w.ns_new_max) return kSlideAdmitCount;
    const int sl = w.nv - (w.drop ? 1 : 0);   // the new slot: the slid window has sl + 1 poses
    bool named = false;                       // a range row so far names the new slot
    int pairs = 0;                            // new pose-to-pose range rows
    for (int e = 0; e < w.nr_new; ++e) {
        const int32_t v0 = w.new_r_idx[e * 2], v1 = w.new_r_idx[e * 2 + 1];
        const bool ok0 = v0 == sl || (v0 == sl - 1 && v0 >= 0);
        const bool ok1 = v1 < 0 ? v1 >= -w.n_anchors : ((v1 == sl || v1 == sl - 1) && v1 != v0 && w.bw_max >= 1);
        const bool names = v0 == sl || v1 == sl;
        if (!ok0 || !ok1 || (named && !names)) return kSlideAdmitIndex;
        named = named || names;
        pairs += v1 >= 0;
    }
    for (int e = 0; e < w.ns_new; ++e) {
        const int32_t vi = w.new_s_idx[e * 4], vj = w.new_s_idx[e * 4 + 1];
        const bool joins = (vi == sl - 1 && vj == sl) || (vi == sl && vj == sl - 1);
        if (!joins || sl < 1 || w.bw_max < 1) return kSlideAdmitIndex;
    }
    // what the drop leaves
    int r_kept = w.nr, p_kept = w.np, s_kept = w.ns;
    if (w.drop) {
        r_kept = 0; p_kept = 0; s_kept = 0;
        for (int e = 0; e < w.nr; ++e) r_kept += w.r_idx[e * 2] != 0 && w.r_idx[e * 2 + 1] != 0;
        for (int e = 0; e < w.np; ++e) p_kept += w.p_idx[e] != 0;
        for (int e = 0; e < w.ns; ++e) s_kept += w.s_idx[e * 4] != 0 && w.s_idx[e * 4 + 1] != 0;
    }
    if (sl + 1 > w.nv_max) return kSlideAdmitNvMax;
    if (r_kept + w.nr_new > w.nr_max) return kSlideAdmitNrMax;
    if (p_kept + w.np_new > w.np_max) return kSlideAdmitNpMax;
    if (s_kept + w.ns_new > w.ns_max) return kSlideAdmitNsMax;
    if (w.pair_rule == kSlidePairsWave6 && (w.ns_new > 0 || pairs > 1)) return kSlideAdmitPairs;
    if (w.pair_rule == kSlidePairsWave6S && (w.ns_new > 1 || pairs > 1)) return kSlideAdmitPairs;
    return kSlideAdmitOk;
}

}  // namespace locamd
