// The per-window half of what loc_window_upload does on the host before anything is launched, stated once for the host and the device
// (loc_window_upload_dev; DESIGN.md §2, "Upload from device arrays") in slide_admit.h's way: plain C++ over ONE window's counts, its index
// tables and the value columns the structure verdict reads — no HIP types, no allocation, no library call.  window_admit_kernel.hip restates
// both functions lane-parallel (rows over lanes, ballots for "any"); tests/host/window_admit_driver.cpp holds a loop over them to
// window_structure.cpp's batch passes (check_instances, chain_scan, translation_only, max_anchor_referenced), which stay as they are.
//
// window_admit: the code of check_instances' FIRST failing check, in its order —
//   1  a count outside [0, nv_max] / [0, nr_max] / [0, np_max] / [0, ns_max]
//   2  a range row's index: v0 outside [0, nv), v1 outside [-n_anchors, nv), v0 == v1            (row by row: a row's 2 comes before its 3,
//   3  a pose-to-pose range row further apart than bw_max                                         and row e's 3 before row e + 1's 2)
//   4  a prior row's pose outside [0, nv)
//   5  an EdgeSE3 row's index: vi or vj outside [0, nv), vi == vj                                 (row by row, as 2 / 3)
//   6  an EdgeSE3 row further apart than bw_max
// 0: admitted.  The counts come first: no row at or beyond a count is ever read, and no row before all four counts are in range.
//
// window_structure_flags: an ADMITTED window's contributions to chain_scan(ordered = true), to translation_only (with and without
// skip_prior_diagonal) and to max_anchor_referenced, as one word: the bits below in the low half, the largest anchor referenced (as -v1,
// 0: none) in the high half.  The batch's verdict is the AND of kWinChain, kWinSingleL, kWinSingleR, kWinSingleS, kWinTransOnly and
// kWinTransOnlySkip, the OR of kWinAnyS and the maximum of the high halves (window_flags_* below).  The pair bits (kWinSingle*) mean something
// for chain windows only — chain_scan stops at the first broken window — and are 0 for every other window.
// translation_only's traps, restated as they are: the nine rotation doubles of a pose and of a prior's measurement are compared BY BITS with
// the identity (std::memcmp: -0.0 is not 0.0 there); lever arms and the prior's rotation information BY VALUE (-0.0 == 0.0 passes, NaN does
// not); a window with an EdgeSE3 row, with more than 1 048 575 poses, or any window under more than 500 000 anchors is not translation-only
// (chain3's packed endpoint word).  s_val is never read.
#pragma once
#include <cstddef>
#include <cstdint>

#include "slide_admit.h"

namespace locamd {

enum WindowAdmit : int {
    kWinAdmitOk = 0, kWinAdmitCounts = 1, kWinAdmitRangeIndex = 2, kWinAdmitRangeWidth = 3, kWinAdmitPriorIndex = 4, kWinAdmitSe3Index = 5,
    kWinAdmitSe3Width = 6
};
enum WindowFlag : uint32_t {
    kWinChain = 1u,           // every pose-to-pose edge joins consecutive slots; edges in the order of their later pose, priors in pose order
    kWinSingleL = 2u,         // no EdgeSE3 row and no second range row on a pair            (batch_topology's single_pairs = AND)
    kWinSingleR = 4u,         // no second range row on a pair
    kWinSingleS = 8u,         // no second EdgeSE3 row on a pair                             (se3_pairs = OR any_s, AND single_r, AND single_s)
    kWinAnyS = 16u,           // the window has an EdgeSE3 row
    kWinTransOnly = 32u,      // translation_only(.., skip_prior_diagonal = false)
    kWinTransOnlySkip = 64u,  // translation_only(.., skip_prior_diagonal = true)
    kWinAndBits = kWinChain | kWinSingleL | kWinSingleR | kWinSingleS | kWinTransOnly | kWinTransOnlySkip,
    kWinOrBits = kWinAnyS
};

// the handle's capacities and the anchor table's size at call time
struct WindowAdmitCaps { int nv_max, nr_max, np_max, ns_max, bw_max, n_anchors; };

LOCAMD_SLIDE_HD inline int window_admit(const WindowAdmitCaps& c, const int32_t* counts, const int32_t* r_idx, const int32_t* p_idx, const int32_t* s_idx) {
    const int32_t nv = counts[0], nr = counts[1], np = counts[2], ns = counts[3];
    if (nv < 0 || nv > c.nv_max || nr < 0 || nr > c.nr_max || np < 0 || np > c.np_max || ns < 0 || ns > c.ns_max) return kWinAdmitCounts;
    for (int e = 0; e < nr; ++e) {
        const int32_t v0 = r_idx[(size_t)e * 2], v1 = r_idx[(size_t)e * 2 + 1];
        if (v0 < 0 || v0 >= nv || v1 >= nv || v1 < -c.n_anchors || v0 == v1) return kWinAdmitRangeIndex;
        if (v1 >= 0 && (v0 - v1 > c.bw_max || v1 - v0 > c.bw_max)) return kWinAdmitRangeWidth;
    }
    for (int e = 0; e < np; ++e) {
        const int32_t v = p_idx[e];
        if (v < 0 || v >= nv) return kWinAdmitPriorIndex;
    }
    for (int e = 0; e < ns; ++e) {
        const int32_t vi = s_idx[(size_t)e * 4], vj = s_idx[(size_t)e * 4 + 1];
        if (vi < 0 || vi >= nv || vj < 0 || vj >= nv || vi == vj) return kWinAdmitSe3Index;
        if (vi - vj > c.bw_max || vj - vi > c.bw_max) return kWinAdmitSe3Width;
    }
    return kWinAdmitOk;
}

// An admitted window (window_admit returned 0: every index below is a pose slot of the window or an anchor code of the table).
// poses [nv][12], r_val [nr][5], p_val [np][18]: read only while a translation-only verdict is still open.
LOCAMD_SLIDE_HD inline uint64_t window_structure_flags(const WindowAdmitCaps& c, const int32_t* counts, const int32_t* r_idx, const int32_t* p_idx, const int32_t* s_idx,
                                                      const double* poses, const double* r_val, const double* p_val) {
    const int32_t nv = counts[0], nr = counts[1], np = counts[2], ns = counts[3];
    // ---- chain_scan(ordered = true), one window ----
    bool chain = true, dup_r = false, dup_s = false;
    int last = 0;   // (poses are numbered from 0, so a later pose of 0 is no pair: `last` = 0 matches nothing)
    for (int e = 0; e < ns; ++e) {
        const int32_t vi = s_idx[(size_t)e * 4], vj = s_idx[(size_t)e * 4 + 1];
        const int key2 = vj > vi ? vj : vi;
        if (key2 < last || (vi - vj != 1 && vj - vi != 1)) chain = false;
        if (key2 == last) dup_s = true;
        last = key2;
    }
    last = 0;
    int last_pair = -1;   // the later pose of the most recent POSE-TO-POSE row (anchor rows in between do not reset it)
    int max_anchor = 0;
    for (int e = 0; e < nr; ++e) {
        const int32_t v0 = r_idx[(size_t)e * 2], v1 = r_idx[(size_t)e * 2 + 1];
        const int key2 = v1 > v0 ? v1 : v0;
        if (key2 < last) chain = false;
        if (v1 >= 0) {
            if (key2 == last_pair) dup_r = true;
            last_pair = key2;
            if (v0 - v1 != 1 && v1 - v0 != 1) chain = false;
        } else if (-v1 > max_anchor) max_anchor = -v1;
        last = key2;
    }
    last = 0;
    for (int e = 0; e < np; ++e) {
        const int32_t v = p_idx[e];
        if (v < last) chain = false;
        last = v;
    }
    uint32_t word = ns != 0 ? kWinAnyS : 0u;
    if (chain) word |= kWinChain | (ns == 0 && !dup_r ? kWinSingleL : 0u) | (!dup_r ? kWinSingleR : 0u) | (!dup_s ? kWinSingleS : 0u);
    // ---- translation_only, one window: what both values of skip_prior_diagonal share, then the priors' rotation information ----
    bool shared = ns == 0 && nv <= 1048575 && c.n_anchors <= 500000, diagonal = true;
    for (int e = 0; e < nr && shared; ++e) {
        const double* v = r_val + (size_t)e * 5;
        if (v[2] != 0.0 || v[3] != 0.0 || v[4] != 0.0) shared = false;
    }
    for (int p = 0; p < nv && shared; ++p) shared = slide_identity_bits(poses + (size_t)p * 12);
    for (int e = 0; e < np && shared; ++e) {
        const double* v = p_val + (size_t)e * 18;
        if (!slide_identity_bits(v)) shared = false;
        else if (v[15] != 0.0 || v[16] != 0.0 || v[17] != 0.0) diagonal = false;
    }
    if (shared) word |= kWinTransOnlySkip | (diagonal ? kWinTransOnly : 0u);
    return (uint64_t)word | ((uint64_t)(uint32_t)max_anchor << 32);
}

// ---- the batch's verdict from the windows' words: AND, OR and maximum, in any order and grouping -------------------------------------------
// One record per batch (and per partial reduction): the lowest-index refused window and its code, the reduced bits, the largest anchor.
struct WindowAdmitRecord {
    long long first_bad;   // the lowest index of a refused window; kWinNoneRefused: every window is admitted
    int32_t code;          // that window's code (0 with kWinNoneRefused)
    uint32_t and_bits;     // AND over the admitted windows' words (all ones for none)
    uint32_t or_bits;      // OR
    int32_t max_anchor;    // max_anchor_referenced over the admitted windows
    int32_t pad[2];
};
constexpr long long kWinNoneRefused = 0x7fffffffffffffffll;

LOCAMD_SLIDE_HD inline WindowAdmitRecord window_record_empty() { return WindowAdmitRecord{kWinNoneRefused, 0, ~0u, 0u, 0, {0, 0}}; }
LOCAMD_SLIDE_HD inline void window_record_add(WindowAdmitRecord& r, long long index, int code, uint64_t word) {
    if (code != kWinAdmitOk) {
        if (index < r.first_bad) { r.first_bad = index; r.code = code; }
        return;
    }
    r.and_bits &= (uint32_t)word; r.or_bits |= (uint32_t)word;
    const int32_t a = (int32_t)(word >> 32);
    if (a > r.max_anchor) r.max_anchor = a;
}
LOCAMD_SLIDE_HD inline void window_record_merge(WindowAdmitRecord& r, const WindowAdmitRecord& o) {
    if (o.first_bad < r.first_bad) { r.first_bad = o.first_bad; r.code = o.code; }
    r.and_bits &= o.and_bits; r.or_bits |= o.or_bits;
    if (o.max_anchor > r.max_anchor) r.max_anchor = o.max_anchor;
}
// chain_scan's three outputs and translation_only's from an admitted batch's record
struct WindowBatchFlags { bool chain, single_pairs, se3_pairs, translation_only, translation_only_skip; };
inline WindowBatchFlags window_batch_flags(const WindowAdmitRecord& r) {
    const uint32_t a = r.and_bits;
    return WindowBatchFlags{(a & kWinChain) != 0, (a & kWinSingleL) != 0, (r.or_bits & kWinAnyS) != 0 && (a & kWinSingleR) != 0 && (a & kWinSingleS) != 0,
                            (a & kWinTransOnly) != 0, (a & kWinTransOnlySkip) != 0};
}

}  // namespace locamd
