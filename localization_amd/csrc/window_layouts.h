// Memory layouts of the window kernels: where every array of one window sits in the dynamic LDS or in its slice of an HBM workspace, how
// long it is, and what the whole comes to.  Each layout is stated ONCE: the kernel walks its pointer through the layout's extents, in the
// layout's order (a walk that cannot leave the layout's total), the host sizes the launch and the allocation by the total, and the fit
// predicates below compare that total with the kernel's limit.  window_lm_kernel alone keeps a pointer walk of its own (window_kernel.hip
// says why); its layout here is what the host sizes it by.  Plain C++17, host and device (LOCAMD_HD is empty without hipcc), so
// tests/host/kernel_layouts_driver.cpp checks every layout on the CPU under sanitizers, offset by offset against a recording of the walks.
//
// Conventions (those of CovLayout): double arrays come first, their offsets counted in doubles from the block's start; the int tables
// follow, their offsets counted in ints from `ints` (itself in doubles).  A Span is {first element, elements}; a Span of 0 elements is an
// array that variant does not have.
#pragma once
#include <stddef.h>

#include "window_kernel.h"

#if defined(__HIPCC__)
#define LOCAMD_HD __host__ __device__
#else
#define LOCAMD_HD
#endif

namespace locamd {

struct Span { size_t at, n; };

// ---- fit limits: dynamic LDS of one workgroup, per kernel ---------------------------------------------------------------------------
constexpr size_t kWave3MaxLds = 64 * 1024;            // wave3_lm_kernel: no opt-in above the default limit
constexpr size_t kWave6MaxLds = 128 * 1024;           // wave6_lm_kernel: per window (one workgroup of one wave)
constexpr size_t kWindowMaxLds = 160 * 1024 - 512;    // window_lm_kernel, one wave per window: the CU's LDS less its static LDS
constexpr size_t kWindowWideStaticLds = 4096;         // >= the static LDS of the several-waves window_lm_kernel (reduction scratch: 2.4 KB)
constexpr size_t kWindowWideMaxLds = 160 * 1024 - kWindowWideStaticLds;
constexpr size_t kArrow3MaxLds = 160 * 1024 - 512;    // arrow3_lm_kernel
constexpr size_t kCovMaxLds = 160 * 1024;             // the four covariance passes (no static LDS)

// ---- wave3_lm_kernel (wave3_kernel.hip) ---------------------------------------------------------------------------------------------
struct W3Layout {
    Span T, rec, ev, fix, pv;     // doubles: W3Lds
    size_t ints;
    Span eidx, epos, pidx;        // ints
    size_t bytes;                 // (the int count rounded up to an even one)
};
LOCAMD_HD inline W3Layout w3_layout(const WindowCaps& c, bool pinfo) {
    W3Layout l;
    size_t p = 0;
    l.T = {p, (size_t)(5 * c.nv_max * 3)}; p += l.T.n;
    l.rec = {p, (size_t)c.nr_max * 16}; p += l.rec.n;
    l.ev = {p, (size_t)c.nr_max * 2}; p += l.ev.n;
    l.fix = {p, (size_t)c.nr_max * 3}; p += l.fix.n;
    l.pv = {p, (size_t)c.np_max * (pinfo ? 9 : 6)}; p += l.pv.n;
    l.ints = p;
    size_t q = 0;
    l.eidx = {q, (size_t)c.nr_max * 2}; q += l.eidx.n;
    l.epos = {q, (size_t)c.nr_max * 2}; q += l.epos.n;
    l.pidx = {q, (size_t)c.np_max}; q += l.pidx.n;
    l.bytes = p * sizeof(double) + ((q + 1) & ~(size_t)1) * sizeof(int);
    return l;
}
LOCAMD_HD inline bool wave3_fits(const WindowCaps& c, bool pinfo) { return c.nv_max <= 64 && w3_layout(c, pinfo).bytes <= kWave3MaxLds; }

// ---- wave6_lm_kernel (wave6_kernel.hip) ---------------------------------------------------------------------------------------------
constexpr int W6_NSLOT = 5;   // pose buffers in LDS: the state + up to four trial states
constexpr int W6_REC = 14;    // per (edge, moving endpoint): w, -w e, the pose's own J (6), the other endpoint's J (6) when that is the previous pose
constexpr int W6_PREC = 27;   // per prior: J^T W J (lower triangle, 21), -J^T W e (6)
struct W6Layout {
    Span pose, rec, prec, ev, fix, pv, sv;   // doubles: W6Lds (sv: with EdgeSE3 records only)
    size_t ints;
    Span eidx, epos, pidx, ppos;             // ints
    size_t bytes;                            // (the int count rounded up to an even one)
};
LOCAMD_HD inline W6Layout w6_layout(const WindowCaps& c, bool se3) {
    W6Layout l;
    size_t p = 0;
    l.pose = {p, (size_t)W6_NSLOT * c.nv_max * 12}; p += l.pose.n;
    l.rec = {p, (size_t)c.nr_max * 2 * W6_REC}; p += l.rec.n;
    l.prec = {p, (size_t)c.np_max * W6_PREC}; p += l.prec.n;
    l.ev = {p, (size_t)c.nr_max * 5}; p += l.ev.n;
    l.fix = {p, (size_t)c.nr_max * 3}; p += l.fix.n;
    l.pv = {p, (size_t)c.np_max * 18}; p += l.pv.n;
    l.sv = {p, se3 ? (size_t)(48 * 64) : 0}; p += l.sv.n;
    l.ints = p;
    size_t q = 0;
    l.eidx = {q, (size_t)c.nr_max * 2}; q += l.eidx.n;
    l.epos = {q, (size_t)c.nr_max * 2}; q += l.epos.n;
    l.pidx = {q, (size_t)c.np_max}; q += l.pidx.n;
    l.ppos = {q, (size_t)c.np_max}; q += l.ppos.n;
    l.bytes = p * sizeof(double) + ((q + 1) & ~(size_t)1) * sizeof(int);
    return l;
}
// se3: the twin with EdgeSE3 records holds one edge per lane and per consecutive pair
LOCAMD_HD inline bool wave6_fits(const WindowCaps& c, bool se3) {
    return c.nv_max <= (se3 ? 63 : 64) && (!se3 || c.ns_max <= 64) && w6_layout(c, se3).bytes <= kWave6MaxLds;
}

// ---- arrow3_lm_kernel (arrow3_kernel.hip) -------------------------------------------------------------------------------------------
constexpr int ARROW_NW = 4;   // waves per instance = segments the chain is cut into at most
struct Arrow3Lds {
    Span PK, GZ, C0, S, bB, xB, xsB, RA, FX, TB, red, AN;   // doubles: ArrowCtx
    size_t bytes;
};
LOCAMD_HD inline Arrow3Lds arrow3_lds_layout(int nv_max, int nb_max) {
    const size_t D = 3 * (size_t)nb_max, D16 = 16 * ((D + 15) / 16);
    Arrow3Lds l;
    size_t p = 0;
    l.PK = {p, (size_t)nv_max * 16}; p += l.PK.n;
    l.GZ = {p, (size_t)nv_max * 12}; p += l.GZ.n;
    l.C0 = {p, D * (D + 1) / 2}; p += l.C0.n;
    l.S = {p, (D + 1) * (D + 2) / 2}; p += l.S.n;
    l.bB = {p, D}; p += D;
    l.xB = {p, D}; p += D;
    l.xsB = {p, D}; p += D;
    l.RA = {p, (size_t)ARROW_NW * D}; p += l.RA.n;
    l.FX = {p, (size_t)ARROW_NW * 4 * D16 * 3}; p += l.FX.n;
    l.TB = {p, 6 * (size_t)nb_max}; p += l.TB.n;
    l.red = {p, 16}; p += 16;
    l.AN = {p, 3 * (size_t)kArrowMaxAnchors}; p += l.AN.n;
    l.bytes = p * sizeof(double);
    return l;
}
// one instance's slice of the HBM workspace: chain translations (two buffers), the stale step, B rows, per-(row, border pose) shares
struct Arrow3Ws {
    Span TT, XS, BB, CS;
    size_t doubles;
};
LOCAMD_HD inline Arrow3Ws arrow3_ws_layout(const WindowCaps& c, int nb_max) {
    Arrow3Ws l;
    size_t p = 0;
    l.TT = {p, (size_t)c.nv_max * 6}; p += l.TT.n;
    l.XS = {p, (size_t)c.nv_max * 3}; p += l.XS.n;
    l.BB = {p, (size_t)c.nv_max * 3 * nb_max * 3}; p += l.BB.n;
    l.CS = {p, (size_t)c.nv_max * nb_max * 9}; p += l.CS.n;
    l.doubles = p;
    return l;
}
LOCAMD_HD inline bool arrow3_fits(const WindowCaps& c, int nb_max) { return arrow3_lds_layout(c.nv_max, nb_max).bytes <= kArrow3MaxLds; }

// ---- window_lm_kernel (window_kernel.hip) -------------------------------------------------------------------------------------------
// Edge records written by the linearisation.  Unary and SE3 edges store their finished CONTRIBUTIONS to the normal equations
// (the 6x6 products are formed once, by the lane that evaluated the edge, from values it holds in registers), so building H
// and b is one load per (edge, entry); diagonal blocks as 21 lower-triangle entries k = r (r + 1) / 2 + c, r >= c.
constexpr int RREC = 16;   // J0[6] J1[6] wr omega_r (+pad): rank-1, expanded on the fly
constexpr int PREC = 28;   // H_vv[21] b_v[6] (+pad)
constexpr int SREC = 90;   // H_ii[21] H_jj[21] H_(later,earlier)[36, column-major like the storage] b_i[6] b_j[6]

// H (lower triangle) and its Cholesky factor are stored by 6x6 blocks.  Capacity: the envelope bound of the caller's bw_max (the exact
// structure of the natural order lies inside it; an elimination order that would need more falls back to the natural one).
LOCAMD_HD inline size_t sky_nnz_bound(int nv, int bw) {
    size_t s = 0;
    for (int v = 0; v < nv; ++v) s += 36 * ((size_t)(v < bw ? v : bw) + 1);
    return s;
}
LOCAMD_HD inline bool window_sparse_path(const WindowCaps& c) { return c.nv_max <= 512; }
// Capacity of H / L in entries.  Windows of 65 .. 512 poses keep them in the HBM workspace, where room is cheap: they get the
// envelope of a band of at least 3, so that a nested-dissection order of a long chain (one fill block per eliminated pose:
// 3 n blocks where the natural order has 2 n) fits and the window factors in ~log2(n) levels instead of n (a 500-pose chain
// of cfg/uwb_pose.yaml's length: 500 levels, 71 ms per solve with the caller's band of 1).
LOCAMD_HD inline size_t window_nnz_capacity(const WindowCaps& c) {
    const int bw = (c.nv_max > 64 && c.nv_max <= 512 && c.bw_max < 3) ? (c.nv_max > 3 ? 3 : c.nv_max - 1) : c.bw_max;
    return sky_nnz_bound(c.nv_max, bw);
}
LOCAMD_HD inline int window_mask_words(const WindowCaps& c) { return c.nv_max <= 64 ? 1 : 8; }

// The structure tables, always in LDS (every address in the sweep and in the edge fold starts with a look-up in them).  The 64-bit mask
// tables first, offsets in 64-bit words; then the int tables.
//   SKYLINE (more than 512 poses): fb, last, boff, ioff;
//   SPARSE, W = 1 or 8 mask words per pose: rowmask, colmask, scr [nv_max][W]; perm, boff, ioff, lvl_col, lvl_blk, colorder; W = 1: otask,
//   one entry per block (8-word windows keep that list in the workspace); W = 8: pushw, rowpre, lvl_mode, dense_off, dense.
struct WindowTables {
    Span rowmask, colmask, scr, pushw;
    size_t ints;   // in 64-bit words
    Span fb, last, rowpre, perm, boff, ioff, lvl_col, lvl_blk, lvl_mode, colorder, dense_off, dense, otask;
    size_t bytes;
};
LOCAMD_HD inline WindowTables window_tables(const WindowCaps& c) {
    const bool sp = window_sparse_path(c);
    const int W = window_mask_words(c);
    const size_t nv = (size_t)c.nv_max, none = 0;
    WindowTables l;
    size_t p = 0, q = 0;
    l.rowmask = {p, sp ? nv * W : none}; p += l.rowmask.n;
    l.colmask = {p, sp ? nv * W : none}; p += l.colmask.n;
    l.scr = {p, sp ? nv * W : none}; p += l.scr.n;
    l.pushw = {p, sp && W > 1 ? (size_t)W : none}; p += l.pushw.n;
    l.ints = p;
    l.fb = {q, sp ? none : nv}; q += l.fb.n;
    l.last = {q, sp ? none : nv}; q += l.last.n;
    l.rowpre = {q, sp && W > 1 ? nv * W : none}; q += l.rowpre.n;
    l.perm = {q, sp ? nv : none}; q += l.perm.n;
    l.boff = {q, nv + 1}; q += l.boff.n;
    l.ioff = {q, nv + 1}; q += l.ioff.n;
    l.lvl_col = {q, sp ? nv + 1 : none}; q += l.lvl_col.n;
    l.lvl_blk = {q, sp ? nv + 1 : none}; q += l.lvl_blk.n;
    l.lvl_mode = {q, sp && W > 1 ? nv + 1 : none}; q += l.lvl_mode.n;
    l.colorder = {q, sp ? nv : none}; q += l.colorder.n;
    l.dense_off = {q, sp && W > 1 ? nv + 2 : none}; q += l.dense_off.n;
    l.dense = {q, sp && W > 1 ? 2 * nv : none}; q += l.dense.n;
    l.otask = {q, sp && W == 1 ? window_nnz_capacity(c) / 36 : none}; q += l.otask.n;
    if (sp && W > 1) q += 1;   // (one int the 8-word tables have always reserved and never used)
    l.bytes = p * 8 + q * sizeof(int);
    return l;
}

// The edge-index tables and incidence lists of one instance (a private writable copy: the SPARSE path relabels them).  Offsets in ints;
// every table starts on a double.  ilist: every edge once per moving endpoint.
struct WindowIndex {
    Span ilist, shared, r_idx, p_idx, s_idx;
    size_t doubles;
};
LOCAMD_HD inline WindowIndex window_index(const WindowCaps& c) {
    WindowIndex l;
    size_t p = 0;   // doubles
    l.ilist = {2 * p, 2 * (size_t)c.nr_max + (size_t)c.np_max + 2 * (size_t)c.ns_max}; p += (l.ilist.n + 1) / 2;
    l.shared = {2 * p, (size_t)c.nr_max + c.ns_max + 1}; p += (l.shared.n + 1) / 2;
    l.r_idx = {2 * p, 2 * (size_t)c.nr_max}; p += (l.r_idx.n + 1) / 2;
    l.p_idx = {2 * p, (size_t)c.np_max}; p += (l.p_idx.n + 1) / 2;
    l.s_idx = {2 * p, 4 * (size_t)c.ns_max}; p += (l.s_idx.n + 1) / 2;
    l.doubles = p;
    return l;
}
// In HBM-workspace mode the index tables move to LDS as well when they are small (every gather starts with a look-up in them; from HBM
// that is a full memory round trip of pure latency)
constexpr size_t INDEX_TABLES_LDS_MAX = 16 * 1024;        // windows of <= 64 poses: keeps 8+ waves per CU
constexpr size_t INDEX_TABLES_LDS_MAX_BIG = 72 * 1024;    // larger windows: their structure tables already limit the CU to 1-2 waves
LOCAMD_HD inline bool window_index_in_lds(const WindowCaps& c) {
    const size_t bytes = window_index(c).doubles * 8;
    if (c.nv_max <= 64) return bytes <= INDEX_TABLES_LDS_MAX;
    return bytes <= INDEX_TABLES_LDS_MAX_BIG && bytes + window_tables(c).bytes + 1024 <= kWindowMaxLds;
}
// 8-word windows: the trailing clique of the elimination order (BASELINE config 4's ten unknown anchors; the last separator of
// a nested dissection in general) is factored as ONE dense supernode of up to ROOT_MAX poses in LDS — when the LDS has room
constexpr int ROOT_MAX = 10;
LOCAMD_HD inline size_t window_root_lds_doubles(const WindowCaps& c) {
    if (!window_sparse_path(c) || window_mask_words(c) == 1) return 0;
    const size_t need = (size_t)(6 * ROOT_MAX + 1) * (6 * ROOT_MAX);
    const size_t used = (window_tables(c).bytes + 7) / 8 * 8 + (window_index_in_lds(c) ? window_index(c).doubles * 8 : 0);
    return used + need * 8 <= kWindowWideMaxLds ? need : 0;
}

// One instance of window_lm_kernel.  global_a: the main arrays in the instance's slice of the HBM workspace (L1/L2-cached), else in LDS.
//   main arrays (doubles from the instance's base): the block-sparse pair, dense vectors, poses, edge records, the index tables' place;
//   workspace mode, SPARSE: the pushed updates and their per-parent sums (28 doubles per column each) and, for 8-word windows, the
//   off-diagonal task list (ints);
//   LDS (doubles from its start): the structure tables; LDS mode: behind the main arrays, followed by the staged edge values and, for
//   one-word windows, the records of the pre-decoded factorisation schedule (stage A: 16-byte records, two per column and one per
//   off-diagonal block plus as many continuation records; stage B: one per block; the hand-out counter); workspace mode: at 0, followed
//   by the index tables when window_index_in_lds and the root supernode when window_root_lds_doubles.
struct WindowLayout {
    WindowTables T;            // from `tables` on
    WindowIndex I;             // from index_lds (LDS) or index_main on
    Span Hs, Ls, diagL, b, x, yrow, pose, bak, rrec, prec, srec;
    size_t index_main;         // the index tables' block behind the main arrays (reserved in both modes)
    Span Us, As, otask_ws;     // otask_ws: in ints from the instance's base
    size_t main_doubles;       // workspace mode: the instance's slice
    size_t tables;             // LDS
    bool index_in_lds;
    size_t index_lds;
    Span r_val, p_val, s_val, recA, recB, rec_count, root;   // recA in doubles (two per record); rec_count: ints from the start of LDS
    size_t recA_cap;
    size_t lds_bytes;
};
LOCAMD_HD inline WindowLayout window_layout(const WindowCaps& c, bool global_a) {
    const bool sp = window_sparse_path(c);
    const int W = window_mask_words(c);
    const size_t nnz = window_nnz_capacity(c), n_max = 6 * (size_t)c.nv_max, nb_max = nnz / 36, none = 0;
    WindowLayout l;
    l.T = window_tables(c); l.I = window_index(c);
    const size_t index = l.I.doubles, tables = (l.T.bytes + 7) / 8;
    size_t p = 0;
    l.Hs = {p, nnz}; p += nnz;
    l.Ls = {p, nnz}; p += nnz;
    l.diagL = {p, n_max}; p += n_max;
    l.b = {p, n_max}; p += n_max;
    l.x = {p, n_max}; p += n_max;
    l.yrow = {p, n_max}; p += n_max;
    l.pose = {p, (size_t)c.nv_max * 12}; p += l.pose.n;
    l.bak = {p, (size_t)c.nv_max * 12}; p += l.bak.n;
    l.rrec = {p, (size_t)c.nr_max * RREC}; p += l.rrec.n;
    l.prec = {p, (size_t)c.np_max * PREC}; p += l.prec.n;
    l.srec = {p, (size_t)c.ns_max * SREC}; p += l.srec.n;
    l.index_main = p; p += index;
    const bool push = global_a && sp;
    l.Us = {p, push ? 28 * (size_t)c.nv_max : none}; p += l.Us.n;
    l.As = {p, push ? 28 * (size_t)c.nv_max : none}; p += l.As.n;
    l.otask_ws = {2 * p, push && W > 1 ? nb_max : none}; p += (l.otask_ws.n + 1) / 2;
    l.main_doubles = p;
    l.recA_cap = sp && W == 1 ? (size_t)c.nv_max + 2 * nb_max : none;
    if (global_a) {
        p = 0;
        l.tables = p; p += tables;
        l.index_in_lds = window_index_in_lds(c);
        l.index_lds = p; if (l.index_in_lds) p += index;
        l.root = {p, window_root_lds_doubles(c)}; p += l.root.n;
        l.r_val = l.p_val = l.s_val = l.recA = l.recB = l.rec_count = {p, 0};
    } else {
        l.tables = p; p += tables;
        l.index_in_lds = false; l.index_lds = l.index_main;
        l.r_val = {p, (size_t)c.nr_max * 5}; p += l.r_val.n;
        l.p_val = {p, (size_t)c.np_max * 18}; p += l.p_val.n;
        l.s_val = {p, (size_t)c.ns_max * 48}; p += l.s_val.n;
        const bool small = sp && W == 1;
        const size_t pad = p & 1;   // 16-byte records
        l.recA = {p + pad, small ? 2 * l.recA_cap : none};
        l.recB = {l.recA.at + l.recA.n, small ? nb_max : none};
        l.rec_count = {2 * (l.recB.at + l.recB.n), small ? (size_t)1 : none};
        if (small) p = l.recB.at + l.recB.n + 1 + (1 - pad);   // (the counter's double, and one for the alignment step whether it is taken or not)
        l.root = {p, 0};
    }
    l.lds_bytes = p * sizeof(double);
    return l;
}
LOCAMD_HD inline bool window_fits(const WindowCaps& c, bool global_a) { return window_layout(c, global_a).lds_bytes <= kWindowMaxLds; }
// windows of more than 64 poses always keep their arrays in the HBM workspace (their structure tables alone fill the LDS)
LOCAMD_HD inline bool window_arrays_in_lds(const WindowCaps& c) { return c.nv_max <= 64 && window_fits(c, false); }

// ---- the covariance passes ----------------------------------------------------------------------------------------------------------
constexpr int kCovChunk = 64;   // edges linearised per pass (one per lane)
constexpr int kCovSRec = 21 + 21 + 36;   // EdgeSE3 record: H_ii, H_jj (lower triangles), the coupling block (rows: the later pose, column-major)

// covariance_kernel.hip: LDS layout of one window (offsets in doubles; the int tables follow the doubles)
struct CovLayout {
    int hd, ho, kb, dg, rrec, prec, srec, ints, ri, pi, si, mk;
    size_t bytes;
};
LOCAMD_HD inline CovLayout cov_layout(int nvl, int D, bool priors, bool se3) {
    CovLayout l;
    const int DD = D * D;
    int p = 0;
    l.hd = p; p += nvl * DD;                   // H_ii -> S_i -> S_i^-1 -> Sigma_i
    l.ho = p; p += nvl * DD;                   // H_{i+1,i} -> K_i
    l.kb = p; p += DD;                         // K_i / T of the current step
    l.dg = p; p += nvl * D;                    // diag(H) of every coordinate (the scale of the relative pivot test)
    l.rrec = p; p += kCovChunk * (1 + 2 * D);  // range: rho' info, J0 (D), J1 (D)
    l.prec = p; if (priors) p += kCovChunk * 21;
    l.srec = p; if (se3) p += kCovChunk * kCovSRec;
    l.ints = p;
    int q = 0;
    l.ri = q; q += 2 * kCovChunk;
    l.pi = q; if (priors) q += kCovChunk;
    l.si = q; if (se3) q += 2 * kCovChunk;
    l.mk = q; q += nvl;
    l.bytes = (size_t)p * sizeof(double) + (size_t)q * sizeof(int);
    return l;
}
LOCAMD_HD inline CovLayout cov_layout(const WindowCaps& c, bool d3) { return cov_layout(c.nv_max, d3 ? 3 : 6, c.np_max > 0, !d3 && c.ns_max > 0); }
LOCAMD_HD inline bool cov_chain_fits(const WindowCaps& c, bool d3) { return cov_layout(c, d3).bytes <= kCovMaxLds; }

// forest_covariance_kernel.hip
constexpr int kFcSe3Chunk = 32;   // EdgeSE3 factors linearised per pass
struct ForestCovLayout {
    int hd, ho, kb, dg, rec, ints, ei, mk, nd, ps;
    size_t bytes;
};
LOCAMD_HD inline ForestCovLayout forest_cov_layout(int nv, bool priors, bool se3) {
    ForestCovLayout l;
    int p = 0;
    l.hd = p; p += nv * 36;   // H_vv -> S_v -> S_v^-1 -> Sigma_v
    l.ho = p; p += nv * 36;   // H_{parent(v),v} -> K_v
    l.kb = p; p += 36;        // the exchange block of the current step
    l.dg = p; p += nv * 6;    // diag(H) of every coordinate (the scale of the relative pivot test)
    int rec = kCovChunk * 13;                                        // range: rho' info, J0 (6), J1 (6)
    if (priors && rec < kCovChunk * 21) rec = kCovChunk * 21;
    if (se3 && rec < kFcSe3Chunk * kCovSRec) rec = kFcSe3Chunk * kCovSRec;
    l.rec = p; p += rec;      // the records of the current chunk (one kind at a time)
    l.ints = p;
    int q = 0;
    l.ei = q; q += 2 * kCovChunk;   // the chunk's pose slots
    l.mk = q; q += nv;
    l.nd = q; q += nv;              // pose slot of the k-th node of the schedule
    l.ps = q; q += nv;              // parent slot of a pose slot (-1: root)
    l.bytes = (size_t)p * sizeof(double) + (size_t)q * sizeof(int);
    return l;
}
LOCAMD_HD inline bool cov_forest_fits(int nv, bool priors, bool se3) { return forest_cov_layout(nv, priors, se3).bytes <= kCovMaxLds; }

// envelope_covariance_kernel.hip
constexpr int kEvThreads = 256;
constexpr int kEvSlots = kEvThreads / 36;          // 7 blocks in flight
constexpr int kEvRangeChunk = 256, kEvPriorChunk = 128, kEvSe3Chunk = 64;   // edges linearised per pass
constexpr int kEvRec = kEvSe3Chunk * kCovSRec;     // doubles of the record region (>= 256 * 13, 128 * 21)
constexpr int kEvLdsRows = kEvRec / 72;            // a column of at most this many rows keeps its two copies (below) in the record region
struct EnvLayout {
    int sinv, rec, ints, ei, wc, first, off, last, list, mk;
    size_t bytes;
};
LOCAMD_HD inline EnvLayout env_layout(int nvm) {
    EnvLayout l;
    int p = 0;
    l.sinv = p; p += 36;       // S_j^-1 of the current column
    l.rec = p; p += kEvRec;    // the records of the current chunk (one kind at a time)
    l.ints = p;
    int q = 0;
    l.ei = q; q += 2 * kEvRangeChunk;   // the chunk's pose slots
    l.wc = q; q += 4;                   // members found by each wave (the ordered compaction of struct(j))
    l.first = q; q += nvm;
    l.off = q; q += nvm + 1;            // first block of row i
    l.last = q; q += nvm;               // the last row that reaches column j
    l.list = q; q += nvm;               // struct(j), ascending
    l.mk = q; q += nvm;
    l.bytes = (size_t)p * sizeof(double) + (size_t)q * sizeof(int);
    return l;
}
LOCAMD_HD inline bool cov_envelope_fits(const WindowCaps& c) { return env_layout(c.nv_max).bytes <= kCovMaxLds; }

// arrow_covariance_kernel.hip
constexpr int kAcThreads = 256;
constexpr int kAcChunk = 256;     // edges linearised per pass (one per thread)
constexpr int kAcBS = 36;         // row stride of B, Y, C: the widest border (12 slots)
constexpr int kAcRec = 7;         // range record: rho' info, J0 (3), J1 (3)
constexpr int kAcRecG = 8;        // its stride in the workspace
struct ArrowCovLayout {
    int hd, ho, dg, cc, ig, rec, ints, ei, cnt, mk, flag;
    size_t bytes;
};
LOCAMD_HD inline ArrowCovLayout arrow_cov_layout(int nvm) {
    ArrowCovLayout l;
    int p = 0;
    l.hd = p; p += nvm * 9;            // H_ii -> S_i^-1 -> [A^-1]_ii -> Sigma_i (chain poses)
    l.ho = p; p += nvm * 9;            // H_{i+1,i} -> K_i
    l.dg = p; p += nvm * 3;            // diag(H) of every coordinate, chain and border (the scale of the relative pivot test)
    l.cc = p; p += kAcBS * kAcBS;      // C -> S -> its Cholesky factor (lower triangle) -> S^-1
    l.ig = p; p += kAcBS;              // reciprocal diagonal of the factor
    l.rec = p; p += kAcChunk * kAcRec; // the records of the current chunk; afterwards L^-1 (36 x 36)
    l.ints = p;
    int q = 0;
    l.ei = q; q += 2 * kAcChunk;       // the chunk's pose slots
    l.cnt = q; q += nvm;               // entries of a chain pose's list
    l.mk = q; q += nvm;
    l.flag = q; q += 2;                // border size; "no pivot failed"
    l.bytes = (size_t)p * sizeof(double) + (size_t)q * sizeof(int);
    return l;
}
LOCAMD_HD inline size_t arrow_cov_ws_doubles(const WindowCaps& c, int cap) {
    return (size_t)c.nr_max * kAcRecG + 2 * (size_t)c.nv_max * 3 * kAcBS + ((size_t)c.nv_max * cap + 1) / 2;
}
LOCAMD_HD inline bool cov_arrow_fits(const WindowCaps& c) { return arrow_cov_layout(c.nv_max).bytes <= kCovMaxLds; }

// The forest kernels' schedule table (window_structure.cpp: build_tree_sched emits it in this order): ts's pointers into a copy of the table
// that starts at base; ts's ten sizes are set.  Returns the table's length in int32s (base to the end of w_kpos).  The host binds the one
// shared table with it (bind_tree_sched), tree_wave_groups_kernel the table of its window's group.
LOCAMD_HD inline size_t tree_sched_bind(TreeSched& ts, const int32_t* base) {
    const int nv = ts.nv, nr = ts.nr, np = ts.np, ns = ts.ns;
    const int32_t* p = base;
    ts.node = p; p += nv; ts.par = p; p += nv;
    ts.r_off = p; p += nv + 1; ts.r_list = p; p += nr;
    ts.p_off = p; p += nv + 1; ts.p_list = p; p += np;
    ts.s_off = p; p += nv + 1; ts.s_list = p; p += ns;
    ts.r_idx = p; p += 2 * nr; ts.s_idx = p; p += 4 * ns;
    ts.w_par = p; p += nv; ts.w_height = p; p += nv;
    ts.w_koff = p; p += nv + 1; ts.w_klist = p; p += nv - ts.nroots;
    ts.w_roff = p; p += nv + 1; ts.w_rlist = p; p += nr;
    ts.w_poff = p; p += nv + 1; ts.w_plist = p; p += np;
    ts.w_soff = p; p += nv + 1; ts.w_slist = p; p += ns;
    ts.w_kleaf = p; p += nv;
    ts.w_ulist = p; p += ts.nu;
    ts.w_kpos = p; p += nv;
    return (size_t)(p - base);
}
// a group's header of a TreeGroups block (window_kernel.h): the ten sizes in TreeSched's order; slot 10: the table's offset, slot 11: its length
LOCAMD_HD inline void tree_group_sizes(TreeSched& ts, const int32_t* h) {
    ts.nv = h[0]; ts.nr = h[1]; ts.np = h[2]; ts.ns = h[3]; ts.depth = h[4]; ts.nroots = h[5]; ts.nlev = h[6]; ts.max_se3_per_node = h[7]; ts.nu = h[8]; ts.max_r_per_node = h[9];
}
// what both launchers of tree_wave_kernel.hip hold a schedule's sizes to (lane = pose: 64 lanes, 64 LDS columns)
LOCAMD_HD inline bool tree_wave_sizes_ok(const TreeSched& ts) { return ts.nv > 0 && ts.nv <= 64 && ts.nlev > 0 && ts.nu >= 0 && ts.nu <= 64; }
// what both launchers of forest_covariance_kernel.hip hold a schedule's sizes to: the LDS blocks are indexed by pose slot and the value tables
// by edge number, so the sizes stay within the handle's capacities, and the window's layout within the covariance passes' LDS limit
LOCAMD_HD inline bool forest_cov_sizes_ok(const TreeSched& ts, const WindowCaps& c) {
    return ts.nv >= 2 && ts.nv <= 64 && ts.nv <= c.nv_max && ts.nr >= 0 && ts.nr <= c.nr_max && ts.np >= 0 && ts.np <= c.np_max && ts.ns >= 0 && ts.ns <= c.ns_max &&
           cov_forest_fits(ts.nv, ts.np > 0, ts.ns > 0);
}
// ... every group of a TreeGroups block, on the host's copy of its headers ([n_groups][kTreeGroupHdr]; a table offset is never negative): the
// dynamic LDS of forest_covariance_kernel<JAC, JOINT, TreeGroups>'s launch — the largest group's layout —, or 0 when a group is refused
LOCAMD_HD inline size_t forest_cov_groups_lds_bytes(const int32_t* host_hdr, int n_groups, const WindowCaps& c) {
    if (!host_hdr || n_groups <= 0) return 0;
    size_t lds = 0;
    for (int k = 0; k < n_groups; ++k) {
        const int32_t* h = host_hdr + (size_t)k * kTreeGroupHdr;
        TreeSched ts{};
        tree_group_sizes(ts, h);
        if (!forest_cov_sizes_ok(ts, c) || h[10] < 0) return 0;
        const size_t b = forest_cov_layout(ts.nv, ts.np > 0, ts.ns > 0).bytes;
        if (b > lds) lds = b;
    }
    return lds;
}

}  // namespace locamd
