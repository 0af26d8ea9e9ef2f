// 6x6 block steps of window_lm_kernel's factorisations (window_kernel.hip), each stated once with its definition, its rounding order and
// what it does at a pivot that is not positive or not finite: the Cholesky factor G of a diagonal block (G G^T = the block, lower), row
// solves against it, the factor's way to and from memory, seven products.  Callers: factor_and_solve (the SKYLINE sweep) and
// root_factor_and_solve (the dense root supernode) take every block step they have from here; factor_and_solve_sparse and
// factor_and_solve_small call wb_sub_update, wb_dot_fms, wb_load_factor and wb_back_solve_scatter.  Their other steps are DELIBERATE
// COPIES of functions in here, kept in window_kernel.hip because the kernel sits at 256 VGPRs and spills, and each of them, made a call,
// moved an instantiation's scratch size or spill counts, or its time beyond the parent's own spread:
//   column mode     wb_chol_left in place with its stores and wb_forward_row: uwb_twist numeric 42.21 .. 42.30 ms against a limit of 42.06;
//                   wb_outer_lower (both sinks), wb_block_blockT_fms, the six wb_forward_row of a block: scratch bytes or SGPR spills;
//   row mode        wb_row_block_sub (three sites): scratch bytes of one instantiation, 204 -> 252;  wb_chol_left from memory,
//                   wb_store_factor_row, wb_forward_row: selfcal 13.62 .. 13.80 ms against 13.55 with G loaded first, SGPR spills of eleven
//                   instantiations with the memory source handed over;
//   back-substitution  wb_blockT_vec_sub and wb_back_solve_gather: pose64 + 0.27 ms with G loaded first, 18.47 .. 18.49 ms against a limit of
//                   18.28 with the factor read in place through callables;
//   small schedule  wb_chol_right, wb_forward_row_scatter, wb_inverse_pivots_finite, wb_blockT_vec_fms: uwb_imu numeric 26.93 .. 26.99 ms
//                   against a limit of 26.92.
// Every copy says so where it stands, DESIGN.md §2 has the table, and tests/test_gpu_window_block_bits.py holds the kernel to the bits it
// had before the first step moved in here: a copy that drifts shows there as a changed digest (a function in here that drifts from its
// copy does not: whoever changes one that has a copy carries the change over, as before).  The SCHEDULE stays
// with the callers — who factors which block, from which memory, between which barriers; in here is only what a lane does to the numbers
// in its registers.
// Conventions: G[r][c], r > c, is the factor's strict lower triangle; ig[j] = 1 / G_jj, the INVERSE pivot (every solve multiplies); a block
// in memory is column-major, entry (r, c) at 6 c + r; a packed update is 27 doubles: the lower triangle at wb_tri(r, c), then 6 of the
// right-hand side (the callers keep one per column, 28 apart).  Every loop is unrolled and every index is static: nothing in here sends a
// register array to scratch memory.  Held to 50-digit references by tests/test_gpu_device_primitives.py (tools/primitives_probe.hip).
// Internal to the including translation unit.
#pragma once
#include "window_device.h"

#include <float.h>
#include <math.h>

namespace locamd {
namespace {

__device__ __forceinline__ constexpr int wb_tri(int r, int c) { return r * (r + 1) / 2 + c; }

// ---- the factor of a diagonal block ----------------------------------------------------------------------------------------------------
// LEFT-LOOKING Cholesky: column j of G from src(r, j) (the raw block's entry, r >= j) minus what the columns before it take,
//   d_j = src(j, j) - sum_{k<j} G_jk^2,   G_jj = sqrt d_j,   G_ij = (src(i, j) - sum_{k<j} G_ik G_jk) / G_jj.
// Rounding: every sum is FMA'd into the source entry, k ascending; 1 / G_jj is sqrt_and_rsqrt's reciprocal after one Newton step
// (1e-16 relative) and G_ij is the product with it.  src: any callable — LDS, the workspace, or G itself (in place: an entry is read before
// it is written).  Pivots: d_j <= 0, NaN or +inf clears ok; the pivot is clamped to 1e-300 before the root, so G and ig stay finite for
// d_j <= 0 and NaN (they mean nothing then: the callers return on !ok) and a positive pivot below 1e-300 is factored as 1e-300.
template <class Src>
__device__ __forceinline__ void wb_chol_left(Src src, double (&G)[6][6], double (&ig)[6], bool& ok) {
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double dj = src(j, j);
#pragma unroll
        for (int k = 0; k < j; ++k) dj = __builtin_fma(-G[j][k], G[j][k], dj);
        ok = ok && (dj > 0.0) && (dj < DBL_MAX);
        double g, igj;
        sqrt_and_rsqrt(fmax(dj, 1e-300), g, igj);
        igj = __builtin_fma(igj, __builtin_fma(-g, igj, 1.0), igj);  // one Newton step: 1/g to ~1e-16
        G[j][j] = g;
        ig[j] = igj;
#pragma unroll
        for (int i2 = j + 1; i2 < 6; ++i2) {
            double v = src(i2, j);
#pragma unroll
            for (int k = 0; k < j; ++k) v = __builtin_fma(-G[i2][k], G[j][k], v);
            G[i2][j] = v * ig[j];
        }
    }
}

// RIGHT-LOOKING Cholesky, in place on the lower triangle of A: per column j the inverse pivot ig_j = pivot_rsqrt(A_jj), the column times
// ig_j, then the trailing lower triangle loses the column's outer product (one FMA per entry).  A's strict lower triangle becomes G; its
// diagonal keeps the pivots d_j.  A second function because it rounds differently from wb_chol_left — an entry is updated column by column
// as the columns finish and the reciprocal root is one cubic step from the hardware seed, with no root of the pivot at all: four dependent
// operations per pivot where the other has a dozen, which is what the latency-bound schedules (small windows, the root supernode) want.
// Pivots: nothing is tested in here.  pivot_rsqrt(d_j) is NaN for d_j < 0 and for NaN (the hardware seed), +inf for d_j = 0, and NaN for
// d_j = +inf as well (the seed is 0, and the step's first product inf * 0 is NaN): ig_j itself is then NaN or inf, which
// wb_inverse_pivots_finite reports; the column and everything after it mean nothing.
__device__ __forceinline__ void wb_chol_right(double (&A)[6][6], double (&ig)[6]) {
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const double g = pivot_rsqrt(A[j][j]);
        ig[j] = g;
#pragma unroll
        for (int i2 = j + 1; i2 < 6; ++i2) A[i2][j] *= g;
#pragma unroll
        for (int i2 = j + 1; i2 < 6; ++i2)
#pragma unroll
            for (int c = j + 1; c <= i2; ++c) A[i2][c] = __builtin_fma(-A[i2][j], A[c][j], A[i2][c]);
    }
}
// wb_chol_right's failure test: the pairwise sum of the six inverse pivots is below DBL_MAX (a pivot <= 0 or not finite left NaN / inf)
__device__ __forceinline__ bool wb_inverse_pivots_finite(const double (&ig)[6]) {
    return ((ig[0] + ig[1]) + (ig[2] + ig[3])) + (ig[4] + ig[5]) < DBL_MAX;
}

// ---- solves against the factor ---------------------------------------------------------------------------------------------------------
// Forward row solve x G^T = s, in place (s becomes x): x_c = (s_c - sum_{k<c} x_k G_ck) ig_c, every term FMA'd into s_c, k ascending, then
// one product.  GATHER form: entry c collects its terms when its turn comes.  No pivot is looked at.
__device__ __forceinline__ void wb_forward_row(double (&s)[6], const double (&G)[6][6], const double (&ig)[6]) {
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        double v = s[c];
#pragma unroll
        for (int k = 0; k < c; ++k) v = __builtin_fma(-s[k], G[c][k], v);
        s[c] = v * ig[c];
    }
}
// the same numbers in SCATTER form (x_c is taken out of the later entries as soon as it exists: the order of wb_chol_right's schedules);
// every entry sees the same FMAs in the same order as in wb_forward_row, so the bits are equal — the instruction order is not
__device__ __forceinline__ void wb_forward_row_scatter(double (&s)[6], const double (&A)[6][6], const double (&ig)[6]) {
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        s[c] *= ig[c];
#pragma unroll
        for (int c2 = c + 1; c2 < 6; ++c2) s[c2] = __builtin_fma(-s[c], A[c2][c], s[c2]);
    }
}
// Back-solve G^T x = t, GATHER form: x_r = (t_r - sum_{s>r} G_sr x_s) ig_r, rows 5 .. 0, every term FMA'd into t_r, s ASCENDING, then one
// product.  fac(s, r) = G_sr and piv(r) = ig_r: any callables, so that a caller whose factor lies in memory reads each entry where it is used.
template <class Fac, class Piv>
__device__ __forceinline__ void wb_back_solve_gather(const double (&t)[6], Fac fac, Piv piv, double (&x)[6]) {
#pragma unroll
    for (int rr = 5; rr >= 0; --rr) {
        double v = t[rr];
#pragma unroll
        for (int s2 = rr + 1; s2 < 6; ++s2) v = __builtin_fma(-fac(s2, rr), x[s2], v);
        x[rr] = v * piv(rr);
    }
}
// the factor in registers
__device__ __forceinline__ void wb_back_solve_gather(const double (&t)[6], const double (&G)[6][6], const double (&ig)[6], double (&x)[6]) {
    wb_back_solve_gather(t, [&](int s2, int rr) { return G[s2][rr]; }, [&](int rr) { return ig[rr]; }, x);
}
// Back-solve G^T x = t, SCATTER form: x_r = t_r ig_r is taken out of the rows above it at once, so row q sees its terms with s DESCENDING:
// other bits than the gather form's, which is why both exist.  t is used up.
__device__ __forceinline__ void wb_back_solve_scatter(double (&t)[6], const double (&G)[6][6], const double (&ig)[6], double (&x)[6]) {
#pragma unroll
    for (int rr = 5; rr >= 0; --rr) {
        x[rr] = t[rr] * ig[rr];
#pragma unroll
        for (int q = 0; q < rr; ++q) t[q] = __builtin_fma(-G[rr][q], x[rr], t[q]);
    }
}

// ---- the factor in memory --------------------------------------------------------------------------------------------------------------
// One lane per row: the lane that holds row `r` (a runtime index) stores G_r0 .. G_r,r-1 at grow[0], grow[st], .. and its inverse pivot at
// *dg.  A ladder over static indices: indexing G by r itself would send the whole array to scratch memory.
__device__ __forceinline__ void wb_store_factor_row(int r, const double (&G)[6][6], const double (&ig)[6], double* grow, int st, double* dg) {
#pragma unroll
    for (int rr = 0; rr < 6; ++rr) {
        if (r == rr) {
#pragma unroll
            for (int c = 0; c < rr; ++c) grow[st * c] = G[rr][c];
            *dg = ig[rr];  // the INVERSE pivot: back-substitution multiplies
        }
    }
}
// the strict lower triangle of the column-major block Gd and the six inverse pivots, into registers
__device__ __forceinline__ void wb_load_factor(const double* Gd, const double* dg, double (&G)[6][6], double (&ig)[6]) {
#pragma unroll
    for (int c = 0; c < 5; ++c)
#pragma unroll
        for (int rr = c + 1; rr < 6; ++rr) G[rr][c] = Gd[6 * c + rr];
#pragma unroll
    for (int c = 0; c < 6; ++c) ig[c] = dg[c];
}

// ---- products --------------------------------------------------------------------------------------------------------------------------
// Two ways to take a product off a target, and they round differently: "_sub" forms the sum of products on its own (an FMA chain from 0,
// k ascending) and subtracts it once; "_fms" FMAs every term into the target.  Neither is replaced by the other anywhere.

// out - sum_k a_k b_k, every term FMA'd into out, k ascending: one entry of a product
__device__ __forceinline__ double wb_dot_fms(const double* a, const double* b, double out) {
#pragma unroll
    for (int k = 0; k < 6; ++k) out = __builtin_fma(-a[k], b[k], out);
    return out;
}
// row times block: S_c -= sum_k li_k B(c, k), B = a block L_JK (entry (c, k) at 6 k + c); li: row i of L_iK, or y_K
__device__ __forceinline__ void wb_row_block_sub(const double (&li)[6], const double* B, double (&S)[6]) {
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) acc = __builtin_fma(li[k], B[6 * k + c], acc);
        S[c] -= acc;
    }
}
// a packed update (a pushed column's L L^T, lower triangle, and L y) taken off a diagonal block and its right-hand side: one subtraction
// per entry
__device__ __forceinline__ void wb_sub_update(double (&G)[6][6], double (&y)[6], const double* U) {
#pragma unroll
    for (int r = 0; r < 6; ++r) {
#pragma unroll
        for (int c = 0; c <= r; ++c) G[r][c] -= U[wb_tri(r, c)];
        y[r] -= U[21 + r];
    }
}
// the lower triangle of B B^T and B y, B = a block L_iK (entry (r, k) at 6 k + r), y = y_K: 27 sums, each an FMA chain from 0 with k
// ascending — what a column owes its parent.  A finished sum goes to put(r, c, sum), c <= r, or to put_rhs(r, sum): the caller subtracts it
// once from its diagonal block and right-hand side ("_sub" rounding), or stores it as a packed update for wb_sub_update to subtract later —
// the same 27 numbers either way.
template <class Put, class PutRhs>
__device__ __forceinline__ void wb_outer_lower(const double (&B)[36], const double (&y)[6], Put put, PutRhs put_rhs) {
#pragma unroll
    for (int r = 0; r < 6; ++r) {
#pragma unroll
        for (int c = 0; c <= r; ++c) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) acc = __builtin_fma(B[6 * k + r], B[6 * k + c], acc);
            put(r, c, acc);
        }
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) acc = __builtin_fma(B[6 * k + r], y[k], acc);
        put_rhs(r, acc);
    }
}
// block times block^T, "_fms": S(r, c) -= sum_k Li(r, k) Lj(c, k), every term FMA'd into S, k ascending; all three column-major.  Li and Lj
// are read from memory a column at a time (the k loop indexes memory only and is left to the compiler).
__device__ __forceinline__ void wb_block_blockT_fms(const double* Li, const double* Lj, double (&S)[36]) {
    for (int k = 0; k < 6; ++k) {
        double li[6], lj[6];
#pragma unroll
        for (int r = 0; r < 6; ++r) { li[r] = Li[6 * k + r]; lj[r] = Lj[6 * k + r]; }
#pragma unroll
        for (int c = 0; c < 6; ++c)
#pragma unroll
            for (int r = 0; r < 6; ++r) S[6 * c + r] = __builtin_fma(-li[r], lj[c], S[6 * c + r]);
    }
}
// block^T times vector, "_sub": t_c -= sum_r B(r, c) x_r, the sum an FMA chain from 0 with r ascending, subtracted once
__device__ __forceinline__ void wb_blockT_vec_sub(const double* B, const double (&x)[6], double (&t)[6]) {
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        double acc = 0.0;
#pragma unroll
        for (int r = 0; r < 6; ++r) acc = __builtin_fma(B[6 * c + r], x[r], acc);
        t[c] -= acc;
    }
}
// block^T times vector, "_fms": every term FMA'd into t_c, r ascending (other bits than wb_blockT_vec_sub's)
__device__ __forceinline__ void wb_blockT_vec_fms(const double* B, const double (&x)[6], double (&t)[6]) {
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) t[c] = __builtin_fma(-B[6 * c + r], x[r], t[c]);
}
}  // namespace
}  // namespace locamd
