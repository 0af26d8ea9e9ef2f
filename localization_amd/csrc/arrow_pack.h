// The arrowhead ("chain + border") rule of arrow3_lm_kernel's tables, stated once for the host and the device in window_admit.h's way: plain
// C++ over ONE window's counts, index tables and the value columns the records take — no HIP types, no allocation, no library call.
// window_structure.cpp's build_arrow_aux is a loop over the two functions below (loc_window_upload, the host path); window_structure_kernel.hip
// restates both lane-parallel for a batch that arrives in device arrays (loc_window_upload_dev under option "upload_dev_structures");
// tests/host/arrow_pack_driver.cpp holds them to build_arrow_aux window by window.
//
// (a) arrow_window_structure: the structure of a window —
//   nb0    the border: the smallest number of LAST pose slots such that every pose-to-pose range between non-consecutive slots has an
//          endpoint there (a max over the range rows); n0 = nv - nb0 chain poses in front of it
//   nseg   the chain is cut into min(max(n0 / 24, 1), 4) segments at the separator poses k n0 / nseg (k = 1 .. nseg - 1), which join the border
//   rows   chain rows [0, nc) = the chain poses that are no separator, in slot order; border rows nc + (0 .. nb): separators first, then the
//          border slots in slot order (nc = n0 - (nseg - 1), nb = nb0 + nseg - 1, nc + nb = nv).  ArrowShape + arrow_row are the `cls` of a pose
//   hdr    [8]  nb, nseg, nc, seg[0 .. 4]: chain rows of segment s are [seg[s], seg[s + 1]); segments nseg .. 3 are empty (= nc)
//   rslot  [nv] the pose slot of row r
//   owner  of a range row: an anchor range belongs to its pose's row; chain-chain to the later chain row (one per consecutive pair);
//          chain-border to the chain row; border-border to the higher border row.  Of a prior row: its pose's row
//   the window's contribution to the batch's nb_max, jmax / jpmax (the most range / prior records any row owns), jch / jpch [16] (the same per
//   chunk of 64 rows, chunks 0 .. 15), list_cap (the most range endpoints and priors any CHAIN pose slot v < n0 has): ArrowMaxima, merged by max
//   and every refusal of build_arrow_aux that one window decides (ArrowRefusal); the batch-level ones are arrow_batch_refused's.
// (b) arrow_window_pack: the record a range / prior row becomes and where it goes — rec [nchunk][jmax][64][3] = code, measurement, information
//   with code = (index << 3) | (kind << 1) | own-is-endpoint-0 (kind 0: fixed anchor `index`; 1: the previous chain row; 2: border pose `index`),
//   prec [nchunk][jpmax][64][7] = 1.0, Z^-1.t (p_val[9 .. 11]), the information's translation diagonal (p_val[12 .. 14]); a row's k-th record is
//   its k-th row IN TABLE ORDER, at [row / 64][k][row % 64]; every slot no record takes is -1.0 (rec, all three doubles) / 0.0 (prec, all seven).
#pragma once
#include <cstddef>
#include <cstdint>

#include "slide_admit.h"

namespace locamd {

constexpr int kArrowPackAnchors = 256;   // = kArrowMaxAnchors (window_kernel.h; window_structure.cpp asserts it): anchor codes from here on are refused
constexpr int kArrowSegments = 4;        // = ARROW_NW (window_layouts.h): the segments the chain is cut into at most
constexpr int kArrowBorderMax = 12;      // nb0 at most
constexpr int kArrowChunks = 16;         // chunks of 64 rows jch / jpch describe

enum ArrowRefusal : int {
    kArrowOk = 0,
    kArrowAnchorCode = 1,   // a range names anchor kArrowPackAnchors or beyond (arrow3_lm_kernel keeps the anchor table in LDS)
    kArrowBorder = 2,       // nb0 < 1 (a chain: no border), nb0 > kArrowBorderMax, or fewer than two chain poses
    kArrowChainGap = 3,     // a chain-chain range between rows that are not neighbours (cannot happen: non-consecutive ranges end in the border)
    kArrowPairTwice = 4,    // a second range on a consecutive chain pair
    kArrowSelfRange = 5     // a range from a pose to itself (check_instances refuses such a row before)
};

struct ArrowShape { int nv, nb0, n0, nseg, nb, nc, sep[kArrowSegments - 1]; };

// requires 1 <= nb0 and nv - nb0 >= 2
LOCAMD_SLIDE_HD inline ArrowShape arrow_shape(int nv, int nb0) {
    ArrowShape s;
    s.nv = nv; s.nb0 = nb0; s.n0 = nv - nb0;
    s.nseg = s.n0 / 24;
    if (s.nseg > kArrowSegments) s.nseg = kArrowSegments;
    if (s.nseg < 1) s.nseg = 1;
    s.nb = nb0 + s.nseg - 1; s.nc = s.n0 - (s.nseg - 1);
    for (int k = 1; k < kArrowSegments; ++k) s.sep[k - 1] = k < s.nseg ? (int)((long long)k * s.n0 / s.nseg) : -1;
    return s;
}
// the shape a window's hdr names (nv = nc + nb)
LOCAMD_SLIDE_HD inline ArrowShape arrow_shape_of(const int32_t* hdr) { return arrow_shape(hdr[0] + hdr[2], hdr[0] - (hdr[1] - 1)); }

// the row of pose slot v in [0, nv): < nc a chain row, else nc + its border index
LOCAMD_SLIDE_HD inline int arrow_row(const ArrowShape& s, int v) {
    if (v >= s.n0) return s.nc + (s.nseg - 1) + (v - s.n0);
    int below = 0;
    for (int k = 0; k < kArrowSegments - 1; ++k) {
        if (k >= s.nseg - 1) break;
        if (v == s.sep[k]) return s.nc + k;
        if (v > s.sep[k]) ++below;
    }
    return v - below;
}

LOCAMD_SLIDE_HD inline void arrow_header(const ArrowShape& s, int32_t* hdr) {
    hdr[0] = s.nb; hdr[1] = s.nseg; hdr[2] = s.nc; hdr[3] = 0;
    for (int k = 1; k <= kArrowSegments; ++k) hdr[3 + k] = k < s.nseg ? s.sep[k - 1] - (k - 1) : s.nc;   // (the chain rows in front of separator k - 1)
}

// the owner row of a range row with admitted indices and its record's code; chain_pair: a chain-chain range (its pair is the owner row's);
// kArrowOk, kArrowChainGap or kArrowSelfRange
struct ArrowOwner { int row; int code; bool chain_pair; int refusal; };
LOCAMD_SLIDE_HD inline ArrowOwner arrow_range_owner(const ArrowShape& s, int v0, int v1) {
    ArrowOwner o{0, 0, false, kArrowOk};
    int kind, idx, own0;
    const int r0 = arrow_row(s, v0);
    if (v1 < 0) { o.row = r0; kind = 0; idx = -1 - v1; own0 = 1; }
    else {
        if (v1 == v0) { o.refusal = kArrowSelfRange; return o; }
        const int r1 = arrow_row(s, v1);
        if (r0 < s.nc && r1 < s.nc) {
            if (r0 - r1 != 1 && r1 - r0 != 1) { o.refusal = kArrowChainGap; return o; }
            o.row = r0 > r1 ? r0 : r1; kind = 1; idx = 0; own0 = r0 > r1; o.chain_pair = true;
        } else if (r0 < s.nc) { o.row = r0; kind = 2; idx = r1 - s.nc; own0 = 1; }
        else if (r1 < s.nc) { o.row = r1; kind = 2; idx = r0 - s.nc; own0 = 0; }
        else { o.row = r0 > r1 ? r0 : r1; kind = 2; idx = (r0 > r1 ? r1 : r0) - s.nc; own0 = r0 > r1; }
    }
    o.code = (idx << 3) | (kind << 1) | own0;
    return o;
}

// a window's contribution to the batch's sizes; the batch's are the maxima (any order and grouping)
struct ArrowMaxima { int32_t nb_max, jmax, jpmax, list_cap, jch[kArrowChunks], jpch[kArrowChunks]; };
LOCAMD_SLIDE_HD inline ArrowMaxima arrow_maxima_empty() {
    ArrowMaxima m;
    m.nb_max = 0; m.jmax = 1; m.jpmax = 1; m.list_cap = 1;
    for (int k = 0; k < kArrowChunks; ++k) { m.jch[k] = 1; m.jpch[k] = 1; }
    return m;
}
LOCAMD_SLIDE_HD inline void arrow_maxima_merge(ArrowMaxima& m, const ArrowMaxima& o) {
    if (o.nb_max > m.nb_max) m.nb_max = o.nb_max;
    if (o.jmax > m.jmax) m.jmax = o.jmax;
    if (o.jpmax > m.jpmax) m.jpmax = o.jpmax;
    if (o.list_cap > m.list_cap) m.list_cap = o.list_cap;
    for (int k = 0; k < kArrowChunks; ++k) {
        if (o.jch[k] > m.jch[k]) m.jch[k] = o.jch[k];
        if (o.jpch[k] > m.jpch[k]) m.jpch[k] = o.jpch[k];
    }
}
// build_arrow_aux's refusals of the whole batch, but arrow3_fits (window_layouts.h), which the caller asks with nb_max
LOCAMD_SLIDE_HD inline bool arrow_batch_refused(const ArrowMaxima& m) { return m.jmax > 64 || m.jpmax > 16 || m.nb_max > 15; }

// (a) One ADMITTED window (window_admit.h / check_instances: every index is a pose slot of the window or an anchor code).  counts [4],
// r_idx [nr][2], p_idx [np]; hdr [8] and rslot [nv] are written (rslot's slots from nv on are the caller's: 0 in build_arrow_aux's tables);
// work [3 nv]: the per-row counters, left in an unspecified state.  m: merged with the window's contribution when the window is taken.
// Returns kArrowOk or the FIRST refusal in the order of ArrowRefusal's passes (anchor codes, the border, then row by row).
LOCAMD_SLIDE_HD inline int arrow_window_structure(const int32_t* counts, const int32_t* r_idx, const int32_t* p_idx, int32_t* hdr, int32_t* rslot, int32_t* work,
                                                  ArrowMaxima& m) {
    const int nv = counts[0], nr = counts[1], np = counts[2];
    int nb0 = 0;
    for (int e = 0; e < nr; ++e) {
        const int v0 = r_idx[2 * e], v1 = r_idx[2 * e + 1];
        if (v1 < 0) {
            if (-1 - v1 >= kArrowPackAnchors) return kArrowAnchorCode;
            continue;
        }
        const int hi = v0 > v1 ? v0 : v1, lo = v0 > v1 ? v1 : v0;
        if (hi - lo != 1 && nv - hi > nb0) nb0 = nv - hi;
    }
    if (nb0 < 1 || nb0 > kArrowBorderMax || nv - nb0 < 2) return kArrowBorder;
    const ArrowShape s = arrow_shape(nv, nb0);
    arrow_header(s, hdr);
    for (int v = 0; v < nv; ++v) rslot[arrow_row(s, v)] = v;
    int32_t *nedge = work, *nprior = work + nv, *pairs = work + 2 * (size_t)nv;
    for (int r = 0; r < nv; ++r) { nedge[r] = 0; nprior[r] = 0; pairs[r] = 0; }
    ArrowMaxima w = arrow_maxima_empty();
    for (int e = 0; e < nr; ++e) {
        const ArrowOwner o = arrow_range_owner(s, r_idx[2 * e], r_idx[2 * e + 1]);
        if (o.refusal != kArrowOk) return o.refusal;
        if (o.chain_pair && ++pairs[o.row] > 1) return kArrowPairTwice;
        const int k = ++nedge[o.row];
        if (k > w.jmax) w.jmax = k;
        if (o.row / 64 < kArrowChunks && k > w.jch[o.row / 64]) w.jch[o.row / 64] = k;
    }
    for (int e = 0; e < np; ++e) {
        const int row = arrow_row(s, p_idx[e]);
        const int k = ++nprior[row];
        if (k > w.jpmax) w.jpmax = k;
        if (row / 64 < kArrowChunks && k > w.jpch[row / 64]) w.jpch[row / 64] = k;
    }
    w.nb_max = s.nb;
    int32_t* deg = work;   // (the row counts are not needed any more) by pose slot: range endpoints and priors
    for (int v = 0; v < nv; ++v) deg[v] = 0;
    for (int e = 0; e < nr; ++e) {
        ++deg[r_idx[2 * e]];
        if (r_idx[2 * e + 1] >= 0) ++deg[r_idx[2 * e + 1]];
    }
    for (int e = 0; e < np; ++e) ++deg[p_idx[e]];
    for (int v = 0; v < s.n0; ++v) if (deg[v] > w.list_cap) w.list_cap = deg[v];
    arrow_maxima_merge(m, w);
    return kArrowOk;
}

// where record k of a row lies in a window's rec / prec (doubles from the window's base)
LOCAMD_SLIDE_HD inline size_t arrow_rec_at(int jmax, int row, int k) { return (((size_t)(row / 64) * jmax + k) * 64 + row % 64) * 3; }
LOCAMD_SLIDE_HD inline size_t arrow_prec_at(int jpmax, int row, int k) { return (((size_t)(row / 64) * jpmax + k) * 64 + row % 64) * 7; }
LOCAMD_SLIDE_HD inline size_t arrow_rec_doubles(int nchunk, int jmax) { return (size_t)nchunk * jmax * 64 * 3; }
LOCAMD_SLIDE_HD inline size_t arrow_prec_doubles(int nchunk, int jpmax) { return (size_t)nchunk * jpmax * 64 * 7; }
LOCAMD_SLIDE_HD inline void arrow_put_range(double* q, int code, const double* rv) { q[0] = (double)code; q[1] = rv[0]; q[2] = rv[1]; }
LOCAMD_SLIDE_HD inline void arrow_put_prior(double* q, const double* pv) {
    q[0] = 1.0;
    for (int k = 0; k < 3; ++k) { q[1 + k] = pv[9 + k]; q[4 + k] = pv[12 + k]; }
}

// (b) One window arrow_window_structure took, whose batch passed arrow_batch_refused with the sizes jmax / jpmax: its records.  hdr [8] as
// written there; r_val [nr][5], p_val [np][18]; rec [arrow_rec_doubles], prec [arrow_prec_doubles] are written completely (the fill included);
// work [2 nv]: the rows' running slots.
LOCAMD_SLIDE_HD inline void arrow_window_pack(const int32_t* counts, const int32_t* hdr, const int32_t* r_idx, const double* r_val, const int32_t* p_idx, const double* p_val,
                                              int nchunk, int jmax, int jpmax, double* rec, double* prec, int32_t* work) {
    const int nv = counts[0], nr = counts[1], np = counts[2];
    const ArrowShape s = arrow_shape_of(hdr);
    const size_t n_rec = arrow_rec_doubles(nchunk, jmax), n_prec = arrow_prec_doubles(nchunk, jpmax);
    for (size_t i = 0; i < n_rec; ++i) rec[i] = -1.0;
    for (size_t i = 0; i < n_prec; ++i) prec[i] = 0.0;
    int32_t *nedge = work, *nprior = work + nv;
    for (int r = 0; r < nv; ++r) { nedge[r] = 0; nprior[r] = 0; }
    for (int e = 0; e < nr; ++e) {
        const ArrowOwner o = arrow_range_owner(s, r_idx[2 * e], r_idx[2 * e + 1]);
        arrow_put_range(rec + arrow_rec_at(jmax, o.row, nedge[o.row]++), o.code, r_val + (size_t)e * 5);
    }
    for (int e = 0; e < np; ++e) {
        const int row = arrow_row(s, p_idx[e]);
        arrow_put_prior(prec + arrow_prec_at(jpmax, row, nprior[row]++), p_val + (size_t)e * 18);
    }
}

// ---- what window_structure_kernel.hip leaves of a batch: AND and maximum, in any order and grouping ------------------------------------------
enum WindowStructBit : uint32_t {
    kStructArrow = 1u,    // every window is an arrowhead (arrow_window_structure returned kArrowOk); the maxima below are the batch's
    kStructEqual0 = 2u    // every window's four counts and used index rows equal window 0's (build_tree_sched's "one topology")
};
struct WindowStructRecord {
    uint32_t and_bits;
    int32_t pad[3];
    ArrowMaxima arrow;   // over the windows that are arrowheads
};
LOCAMD_SLIDE_HD inline WindowStructRecord struct_record_empty() { return WindowStructRecord{~0u, {0, 0, 0}, arrow_maxima_empty()}; }
LOCAMD_SLIDE_HD inline void struct_record_merge(WindowStructRecord& r, const WindowStructRecord& o) {
    r.and_bits &= o.and_bits;
    arrow_maxima_merge(r.arrow, o.arrow);
}

}  // namespace locamd
