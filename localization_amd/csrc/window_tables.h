// The eight tables a batch of windows travels in (window_kernel.h: "Layout of one instance"), described ONCE for the host side:
// capi_window.cpp allocates, stages, uploads and fetches by this description; a new table or a changed record width is an edit here.
#pragma once
#include <cstdint>
#include <cstring>

#include "window_kernel.h"

namespace locamd {

enum WindowTable { kPoses, kCounts, kRVal, kPVal, kSVal, kRIdx, kPIdx, kSIdx, kWindowTables };   // (the order of the staging blocks)

// bytes of ONE instance in table t
inline size_t table_bytes(const WindowCaps& c, int t) {
    const size_t nv = c.nv_max, nr = c.nr_max, np = c.np_max, ns = c.ns_max;
    const size_t bytes[kWindowTables] = {nv * 12 * sizeof(double), 4 * sizeof(int32_t), nr * 5 * sizeof(double), np * 18 * sizeof(double), ns * 48 * sizeof(double),
                                         nr * 2 * sizeof(int32_t), np * sizeof(int32_t), ns * 4 * sizeof(int32_t)};
    return bytes[t];
}

// a caller's batch: n instances and its eight host arrays (pointers only, nothing is owned)
struct HostTables { const void* t[kWindowTables]; };
struct HostBatch {
    int64_t n;
    const double* poses; const int32_t* counts; const double *r_val, *p_val, *s_val; const int32_t *r_idx, *p_idx, *s_idx;   // (WindowTable order)
    HostTables tables() const { return {{poses, counts, r_val, p_val, s_val, r_idx, p_idx, s_idx}}; }
};
// where a kernel finds the tables: eight base pointers the device can read (device arrays, or the page-locked staging block)
struct DeviceTables { void* t[kWindowTables]; };

// One block for n instances: up to eight prefix pieces, then the tables from first_table on in WindowTable order, every piece 16-byte
// aligned; offsets of the pieces, their bytes as given and the block's size.  first_table = kWindowTables: prefix pieces alone.  The solve's
// prefix is [poses | result], which come back as one copy, in front of the tables from kCounts on: tab[kPoses] = pre[0] = 0.
struct BlockLayout { size_t pre[8], len[8], tab[kWindowTables], end; };
inline BlockLayout pack_block(const WindowCaps& c, size_t n, const size_t* prefix_bytes, int n_prefix, int first_table) {
    auto al = [](size_t b) { return (b + 15) & ~(size_t)15; };
    BlockLayout L{};
    for (int k = 0; k < n_prefix; ++k) { L.pre[k] = L.end; L.len[k] = prefix_bytes[k]; L.end += al(prefix_bytes[k]); }
    for (int t = first_table; t < kWindowTables; ++t) { L.tab[t] = L.end; L.end += al(n * table_bytes(c, t)); }
    return L;
}
// ---- every other block of capi_window.cpp, by name (tests/test_window_blocks_cpu.py holds each to the arithmetic it replaced) ----------------
// a covariance call: the outputs [cov | mask | status], then all eight tables; a joint call (npair_max > 0) has
// [cross | pair counts | pairs] between them: a fourth output and two more inputs
inline BlockLayout covariance_layout(const WindowCaps& c, size_t n, size_t npair_max) {
    const size_t nv = c.nv_max, P = npair_max;
    const size_t pre[6] = {n * nv * 36 * sizeof(double), n * nv * sizeof(int32_t), n * sizeof(int32_t), n * P * 36 * sizeof(double), n * sizeof(int32_t), n * P * 2 * sizeof(int32_t)};
    return pack_block(c, n, pre, P ? 6 : 3, kPoses);
}
// the marginal-prior pass: the outputs [slot | prior | grad | shift | rank | status], the input [drop], then all eight tables
inline BlockLayout marginal_prior_layout(const WindowCaps& c, size_t n) {
    const size_t pre[7] = {n * sizeof(int32_t), n * 48 * sizeof(double), n * 6 * sizeof(double), n * 6 * sizeof(double), n * sizeof(int32_t), n * sizeof(int32_t), n * sizeof(int32_t)};
    return pack_block(c, n, pre, 7, kPoses);
}
// the edge audit: the outputs [r_chi2 | p_chi2 | s_chi2 | total | active], then all eight tables
inline BlockLayout edge_audit_layout(const WindowCaps& c, size_t n) {
    const size_t pre[5] = {n * c.nr_max * sizeof(double), n * c.np_max * sizeof(double), n * c.ns_max * sizeof(double), n * sizeof(double), n * sizeof(int32_t)};
    return pack_block(c, n, pre, 5, kPoses);
}
// the pair tables of a resident joint call: [pair counts | pairs]
inline BlockLayout resident_pairs_layout(size_t n, size_t npair_max) {
    const size_t pre[2] = {n * sizeof(int32_t), n * npair_max * 2 * sizeof(int32_t)};
    return pack_block(WindowCaps{}, n, pre, 2, kWindowTables);
}
// the staged inputs of a host slide: [drop | new_r_counts | new_p_counts | new_r_idx | new_pose | new_r_val | new_p_val]
inline BlockLayout slide_inputs_layout(size_t n, size_t nr_new_max, size_t np_new_max) {
    const size_t pre[7] = {n * sizeof(int32_t), n * sizeof(int32_t), n * sizeof(int32_t), n * nr_new_max * 2 * sizeof(int32_t), n * 12 * sizeof(double),
                           n * nr_new_max * 5 * sizeof(double), n * np_new_max * 18 * sizeof(double)};
    return pack_block(WindowCaps{}, n, pre, 7, kWindowTables);
}
// a slide's marginal pass, for the handle's B windows: [drop (zeros) | slot | rank | status | prior | grad | shift]
enum SlideMarginalPiece { kMDrop, kMSlot, kMRank, kMStatus, kMPrior, kMGrad, kMShift };
inline BlockLayout slide_marginal_layout(size_t B) {
    const size_t pre[7] = {B * sizeof(int32_t), B * sizeof(int32_t), B * sizeof(int32_t), B * sizeof(int32_t), B * 48 * sizeof(double), B * 6 * sizeof(double), B * 6 * sizeof(double)};
    return pack_block(WindowCaps{}, B, pre, 7, kWindowTables);
}
// the handle's own outputs of window_message_kernel for B windows (loc_window_push_messages_resident_dev builds here, the slide reads here):
// the eleven arrays of loc_window_message_rows in its order, each 16-byte aligned
enum MessageRowsPiece { kGDrop, kGPose, kGRCounts, kGRIdx, kGRVal, kGPCounts, kGPVal, kGSCounts, kGSIdx, kGSVal, kGVerdict, kMessageRowsPieces };
struct MessageRowsLayout { size_t off[kMessageRowsPieces], end; };
inline MessageRowsLayout message_rows_layout(size_t B) {
    const size_t i4 = sizeof(int32_t), f8 = sizeof(double);
    const size_t bytes[kMessageRowsPieces] = {B * i4, B * 12 * f8, B * i4, B * 2 * 2 * i4, B * 2 * 5 * f8, B * i4, B * 2 * 18 * f8, B * i4, B * 1 * 4 * i4, B * 1 * 48 * f8, B * i4};
    MessageRowsLayout L{};
    for (int k = 0; k < kMessageRowsPieces; ++k) { L.off[k] = L.end; L.end += (bytes[k] + 15) & ~(size_t)15; }
    return L;
}
inline DeviceTables tables_at(char* base, const BlockLayout& L) {
    DeviceTables d;
    for (int t = 0; t < kWindowTables; ++t) d.t[t] = base + L.tab[t];
    return d;
}
// the batch into the host side of a block
inline void stage_tables(char* h, const BlockLayout& L, const WindowCaps& c, const HostBatch& b) {
    const HostTables src = b.tables();
    for (int t = 0; t < kWindowTables; ++t)
        if (const size_t bytes = (size_t)b.n * table_bytes(c, t)) std::memcpy(h + L.tab[t], src.t[t], bytes);
}

}  // namespace locamd
