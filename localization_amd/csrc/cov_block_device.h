// What the window covariance passes do alike (covariance_kernel.hip: chain windows; forest_covariance_kernel.hip: forest windows;
// arrow_covariance_kernel.hip: arrowhead windows): the per-edge records of the linearisation (range, unary prior, the
// EdgeSE3 record's layout), the rule for excluded coordinates, the relative pivot rule behind LOC_ERR_SINGULAR (cov_pivot_above_noise:
// all three passes), and the block steps of the two wave-per-window passes — the register Cholesky with its pivot tests and L^-1
// (cov_chol_inverse), the elimination of one block, the K^T Sigma K update and the store; the chain is the forest with parent = next
// pose.  (The arrowhead pass keeps its one-lane 3 x 3 loops: DESIGN.md §4.)  Internal to the including translation unit.
#pragma once
#include "se3_edge_device.h"
#include "cov_device.h"
#include "window_layouts.h"

#include <float.h>
#include <math.h>

namespace locamd {
namespace {

#define LOCAMD_CV_TRI(r, c) ((r) >= (c) ? (r) * ((r) + 1) / 2 + (c) : (c) * ((c) + 1) / 2 + (r))

// one unary EdgeSE3Prior at X: its J^T W J (lower triangle, 21) — se3_edge_device.h: prior_terms, prior_diag_hessian
__device__ __forceinline__ void cov_prior_block(const double* val, const double* X, double* rec) {
    double err[6], J[36];
    prior_terms<true>(val, X, err, J);
    prior_diag_hessian(J, val + 12, rec);
}

// the same with the prior's full information matrix W (6x6 row-major, symmetric: loc_window_set_prior_information) in the place of val's
// diagonal — window_device.h: prior_full_hessian, as window_kernel.hip's evaluate_edges<.., PINFO>; the record's layout is the same
__device__ __forceinline__ void cov_prior_block_full(const double* val, const double* W, const double* X, double* rec) {
    double err[6], J[36];
    prior_terms<true>(val, X, err, J);
    prior_full_hessian(J, W, rec);
}

// the chain 3 x 3 pass under a structured table (covariance_kernel<3, .., true>): the prior's R_E^T W R_E with the dense 3 x 3 block W of
// its table row (prior3_load / prior3_mul_add: window_device.h, shared with wave3_lm_kernel<JAC, true>), lower triangle into rec[0 .. 5] —
// cov_prior_block's layout for r, c < 3.  (R_E is the identity in a translation-only batch: the block is W itself, as the diagonal
// form's is diag(W).)
__device__ __forceinline__ void cov_prior_block3(const double* val, const double* W36, const double* X, double* rec) {
    double RE[9], w[6];
    mat_mul(val, X, RE);
    prior3_load(W36, w);
#pragma unroll
    for (int cc = 0; cc < 3; ++cc) {
        const double col[3] = {RE[cc], RE[3 + cc], RE[6 + cc]};
        double t[3] = {0.0, 0.0, 0.0};
        prior3_mul_add(w, col, t);   // W R_E[:, cc]
#pragma unroll
        for (int r = cc; r < 3; ++r) {
            double h = 0.0;
#pragma unroll
            for (int i = 0; i < 3; ++i) h += RE[i * 3 + r] * t[i];
            rec[r * (r + 1) / 2 + cc] = h;
        }
    }
}

// one range edge (no lever arm on endpoint 1): rho' info, J0 (D columns of the pose carrying the lever arm), J1 (D columns of the other pose)
// err_out: where the marginal-prior pass wants the edge's error as well (the covariance passes pass none)
template <int D, int JAC>
__device__ __forceinline__ void cov_range_rec(const double* X0, const double* X1, const double* p1, bool pose1, const double* val, double* rec, double* err_out = nullptr) {
    const double meas = val[0], info = val[1];
    const double off[3] = {val[2], val[3], val[4]};
    double J0[6] = {0, 0, 0, 0, 0, 0}, J1[6] = {0, 0, 0, 0, 0, 0};
    double err;
    if (JAC == 0) {
        double p0[3];
        mat_vec(X0, off, p0);
        double u[3] = {(p0[0] + X0[9]) - p1[0], (p0[1] + X0[10]) - p1[1], (p0[2] + X0[11]) - p1[2]};
        const double n = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
        err = meas - n;
        const double inv = n > 0.0 ? 1.0 / n : 0.0;   // coincident endpoints: J = 0 (what the central difference gives)
        u[0] *= inv; u[1] *= inv; u[2] *= inv;
        double uR[3];
        mat_tvec(X0, u, uR);
        J0[0] = -uR[0]; J0[1] = -uR[1]; J0[2] = -uR[2];
        J0[3] = 2.0 * (uR[1] * off[2] - uR[2] * off[1]);   // dp0/dv = -2 R0 [o]x  =>  de/dv0 = 2 (uR x o)
        J0[4] = 2.0 * (uR[2] * off[0] - uR[0] * off[2]);
        J0[5] = 2.0 * (uR[0] * off[1] - uR[1] * off[0]);
        if (pose1) {
            double uR1[3];
            mat_tvec(X1, u, uR1);
            J1[0] = uR1[0]; J1[1] = uR1[1]; J1[2] = uR1[2];
        }
    } else {
        err = range_error_plain(X0, X0 + 9, off, p1, meas);
        J0[0] = range_jac_numeric<0>(X0, off, X1, p1, 0, meas);
        J0[1] = range_jac_numeric<1>(X0, off, X1, p1, 0, meas);
        J0[2] = range_jac_numeric<2>(X0, off, X1, p1, 0, meas);
        if (D == 6) {
            J0[3] = range_jac_numeric<3>(X0, off, X1, p1, 0, meas);
            J0[4] = range_jac_numeric<4>(X0, off, X1, p1, 0, meas);
            J0[5] = range_jac_numeric<5>(X0, off, X1, p1, 0, meas);
        }
        if (pose1) {   // (without a lever arm, rotating endpoint 1 does not move its point: those columns are exactly 0)
            J1[0] = range_jac_numeric<0>(X0, off, X1, p1, 1, meas);
            J1[1] = range_jac_numeric<1>(X0, off, X1, p1, 1, meas);
            J1[2] = range_jac_numeric<2>(X0, off, X1, p1, 1, meas);
        }
    }
    const double chi = err * (info * err);
    rec[0] = (1.0 / (1.0 + chi)) * info;   // rho' Omega
    if (err_out) *err_out = err;
#pragma unroll
    for (int k = 0; k < D; ++k) { rec[1 + k] = J0[k]; rec[1 + D + k] = J1[k]; }
}

// one range edge (v0, v1) of a window with poses P: endpoint 1 is pose v1, or the fixed anchor -1 - v1 (identity rotation); the record of cov_range_rec
template <int D, int JAC>
__device__ __forceinline__ void cov_range_edge(const double* P, const double* anchors, int v0, int v1, const double* val, double* rec, double* err_out = nullptr) {
    double X0[12], X1[12], p1[3];
#pragma unroll
    for (int k = 0; k < 12; ++k) X0[k] = P[v0 * 12 + k];
    const int v1c = v1 >= 0 ? v1 : v0;
#pragma unroll
    for (int k = 0; k < 12; ++k) X1[k] = P[v1c * 12 + k];
    if (v1 >= 0) { p1[0] = X1[9]; p1[1] = X1[10]; p1[2] = X1[11]; }
    else { const double* an = anchors + (size_t)(-1 - v1) * 3; p1[0] = an[0]; p1[1] = an[1]; p1[2] = an[2]; }
    cov_range_rec<D, JAC>(X0, X1, p1, v1 >= 0, val, rec, err_out);
}

// excluded coordinates of pose `v`'s assembled diagonal block: a diagonal entry exactly 0 (its row and column are 0 as well) is taken as
// 1 and gets its mask bit; dgv: diag(H) of the pose's coordinates (the scale of the relative pivot test).  Returns the mask.
template <int D>
__device__ __forceinline__ int cov_exclude_zero_diagonal(double* Hv, double* dgv) {
    int bits = D == 3 ? 0x38 : 0;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        if (Hv[k * D + k] == 0.0) { bits |= 1 << k; Hv[k * D + k] = 1.0; }
        dgv[k] = Hv[k * D + k];
    }
    return bits;
}

// ---- the block steps ------------------------------------------------------------------------------------------------------------------
// the relative half of the pivot rule: a pivot at most kCovRelPivot of its coordinate's diagonal entry of H is numerically
// singular (a rank-deficient H leaves pivots of rounding size, 1e-16 .. 1e-14 of it, and of either sign: the absolute test alone would pass
// half of them); NaN fails as well
__device__ __forceinline__ bool cov_pivot_above_noise(double pivot, double diag) { return pivot > kCovRelPivot * diag; }

// Cholesky of one D x D block in the thread's registers, pivots checked, and the inverse of its factor.  A: the block (row-major, its lower
// triangle is read); dgv: diag(H) of its coordinates; Li: L^-1 (its lower triangle is written).  ok: cleared by a pivot that is not finite,
// not positive or not above the noise of its coordinate.  No LDS writes, no barriers.
template <int D>
__device__ __forceinline__ void cov_chol_inverse(const double* A_, const double* dgv, bool& ok, double (&Li)[D][D]) {
    double A[D][D];
#pragma unroll
    for (int cc = 0; cc < D; ++cc)
#pragma unroll
        for (int rr = cc; rr < D; ++rr) A[rr][cc] = A_[rr * D + cc];
    double ig[D];
#pragma unroll
    for (int j = 0; j < D; ++j) {
        ok = ok && cov_pivot_above_noise(A[j][j], dgv[j]);
        const double g = pivot_rsqrt(A[j][j]);
        ig[j] = g;
#pragma unroll
        for (int i2 = j + 1; i2 < D; ++i2) A[i2][j] *= g;
#pragma unroll
        for (int i2 = j + 1; i2 < D; ++i2)
#pragma unroll
            for (int cc = j + 1; cc <= i2; ++cc) A[i2][cc] = __builtin_fma(-A[i2][j], A[cc][j], A[i2][cc]);
    }
    double sg = 0.0;
#pragma unroll
    for (int j = 0; j < D; ++j) sg += ig[j];
    ok = ok && sg < DBL_MAX;   // (a pivot <= 0 or not finite: NaN / inf — window_kernel.hip's test)
    // L^-1 (lower): diagonal ig, below it -ig_i sum_k L_ik Linv_kc
#pragma unroll
    for (int cc = 0; cc < D; ++cc) {
        Li[cc][cc] = ig[cc];
#pragma unroll
        for (int rr = cc + 1; rr < D; ++rr) {
            double s = 0.0;
#pragma unroll
            for (int k = cc; k < rr; ++k) s = __builtin_fma(A[rr][k], Li[k][cc], s);
            Li[rr][cc] = -ig[rr] * s;
        }
    }
}

// The wave-per-window passes, lane = entry (r, c) of a D x D block (ent: the lane has one).  Chain windows: parent = the next pose.
// Eliminates node i (pose slot i of the window's LDS blocks: Hd = diagonal blocks, Ho = the blocks H_{parent,node} with the parent's rows, dg =
// diag(H)): Hd[i] holds S_i, the node's diagonal block minus its children's shares.  Every lane factors S_i (cov_chol_inverse) in its
// registers; S_i^-1 = L^-T L^-1 replaces S_i.  With a parent (slot ip): K_i = H_{ip,i} S_i^-1 replaces Ho[i] and Hd[ip] loses K_i H_{i,ip}.
// Kb: one D x D exchange block.  ok: cleared by a failed pivot.
template <int D>
__device__ __forceinline__ void cov_eliminate_block(double* Hd, double* Ho, const double* dg, double* Kb, int i, bool has_parent, int ip, int lane, int r, int c, bool ent, bool& ok) {
    constexpr int DD = D * D;
    double Li[D][D];
    cov_chol_inverse<D>(Hd + i * DD, dg + i * D, ok, Li);
    double sinv = 0.0;   // entry (r, c) of S_i^-1 = L^-T L^-1
    if (ent) {
#pragma unroll
        for (int k = 0; k < D; ++k)
            if (k >= r && k >= c) sinv = __builtin_fma(Li[k][r], Li[k][c], sinv);
    }
    __syncthreads();
    if (ent) Hd[i * DD + lane] = sinv;
    __syncthreads();
    if (has_parent) {
        double kr = 0.0;   // K_i = H_{ip,i} S_i^-1
        if (ent) {
#pragma unroll
            for (int k = 0; k < D; ++k) kr = __builtin_fma(Ho[i * DD + r * D + k], Hd[i * DD + k * D + c], kr);
            Kb[lane] = kr;
        }
        __syncthreads();
        double s = 0.0;    // (K_i H_{i,ip})_rc = sum_k K_rk H_{ip,i}[c][k]
        if (ent) {
#pragma unroll
            for (int k = 0; k < D; ++k) s = __builtin_fma(Kb[r * D + k], Ho[i * DD + c * D + k], s);
        }
        __syncthreads();
        if (ent) { Ho[i * DD + lane] = kr; Hd[ip * DD + lane] -= s; }
        __syncthreads();
    }
}

// selected inversion, node i with parent ip: Sigma_i = S_i^-1 + K_i^T Sigma_ip K_i (Hd[i]: S_i^-1 in, Sigma_i out; Hd[ip]: the parent's finished
// Sigma; Ho[i]: K_i)
template <int D>
__device__ __forceinline__ void cov_back_substitute_block(double* Hd, const double* Ho, double* Kb, int i, int ip, int lane, int r, int c, bool ent) {
    constexpr int DD = D * D;
    if (ent) {
        double t = 0.0;   // T = Sigma_ip K_i
#pragma unroll
        for (int k = 0; k < D; ++k) t = __builtin_fma(Hd[ip * DD + r * D + k], Ho[i * DD + k * D + c], t);
        Kb[lane] = t;
    }
    __syncthreads();
    if (ent) {
        double s = Hd[i * DD + lane];
#pragma unroll
        for (int k = 0; k < D; ++k) s = __builtin_fma(Ho[i * DD + k * D + r], Kb[k * D + c], s);
        Hd[i * DD + lane] = s;
    }
    __syncthreads();
}

// output of window `inst`: symmetric 6x6 per slot ((a + a^T) / 2), excluded rows / columns 0, slots >= nv 0, NaN for a singular window
template <int D>
__device__ __forceinline__ void cov_store_window(const double* Hd, const int* mk, int nv, int nvm, bool ok, int lane, long long inst, double* cov, int32_t* mask, int32_t* status) {
    constexpr int DD = D * D;
    double* out = cov + (size_t)inst * nvm * 36;
    for (int k = lane; k < nvm * 36; k += 64) {
        const int v = k / 36, rr = (k % 36) / 6, cc = k % 6;
        double x = 0.0;
        if (v < nv) {
            if (!ok) x = __builtin_nan("");
            else if (rr < D && cc < D && !((mk[v] >> rr) & 1) && !((mk[v] >> cc) & 1))
                x = (Hd[v * DD + rr * D + cc] + Hd[v * DD + cc * D + rr]) * 0.5;
        }
        out[k] = x;
    }
    for (int v = lane; v < nvm; v += 64) mask[(size_t)inst * nvm + v] = v < nv ? mk[v] : 0;
    if (lane == 0) status[inst] = ok ? 0 : -6;   // LOC_OK / LOC_ERR_SINGULAR
}

// ---- cross blocks (joint covariance calls) ----------------------------------------------------------------------------------------------
// one step down a tree: Sigma_{v,x} = -K_v^T Sigma_{parent(v),x} (Kv = Ho[v]: K_v, rows: the parent; Kb: the running block, replaced)
template <int D>
__device__ __forceinline__ void cov_cross_step(const double* Kv, double* Kb, int lane, int r, int c, bool ent) {
    double s = 0.0;
    if (ent) {
#pragma unroll
        for (int k = 0; k < D; ++k) s = __builtin_fma(Kv[k * D + r], Kb[k * D + c], s);
    }
    __syncthreads();
    if (ent) Kb[lane] = -s;
    __syncthreads();
}

// The cross blocks of window `inst` after the downward sweep of a wave-per-window pass (Hd: Sigma_v, Ho: K_v), lane = entry (r, c):
//   Sigma_ij = M_i Sigma_aa M_j^T,  a = the lowest common ancestor of i and j,  M_i = the product of -K^T along the path i -> a
// (the identity for i = a; no common ancestor: exact zeros).  One running D x D block in Kb: Sigma_aa, down to i, transposed, down to j.
// parent(v): the parent's pose slot, -1 for a root (a chain: v + 1).  The pair is computed as (min, max) and transposed for the other
// order; (i, i) is the symmetrised block cov_store_window writes.  Every walk is bounded by nv.  Uniform over the wave.
template <int D, class Parent>
__device__ __forceinline__ void cov_store_cross(const double* Hd, const double* Ho, double* Kb, const int* mk, int nv, bool ok, int lane, int r, int c,
                                                bool ent, long long inst, const CovPairs& pp, Parent parent) {
    constexpr int DD = D * D;
    const int npr = pp.counts[inst];
    const int32_t* pr = pp.pairs + (size_t)inst * pp.npair_max * 2;
    double* out = pp.cross + (size_t)inst * pp.npair_max * 36;
    for (int p = 0; p < pp.npair_max; ++p) {
        const int pi = p < npr ? pr[2 * p] : -1, pj = p < npr ? pr[2 * p + 1] : -1;
        if (pi < 0 || pi >= nv || pj < 0 || pj >= nv || !ok) {   // an unused slot: 0; a singular window: NaN
            if (lane < 36) out[p * 36 + lane] = (p < npr && !ok) ? __builtin_nan("") : 0.0;
            continue;
        }
        const int i = min(pi, pj), j = max(pi, pj);
        int di = 0, dj = 0;   // depths
        for (int v = parent(i); v >= 0 && di < nv; v = parent(v)) ++di;
        for (int v = parent(j); v >= 0 && dj < nv; v = parent(v)) ++dj;
        int a = i, b = j, hi = 0, hj = 0;   // the steps from i / j up to the common ancestor
        for (; di - hi > dj - hj; ++hi) a = parent(a);
        for (; dj - hj > di - hi; ++hj) b = parent(b);
        for (int k = 0; k < nv && a != b && a >= 0 && b >= 0; ++k) { a = parent(a); b = parent(b); ++hi; ++hj; }
        const bool joined = a >= 0 && a == b;
        __syncthreads();
        if (ent) Kb[lane] = joined ? (Hd[a * DD + r * D + c] + Hd[a * DD + c * D + r]) * 0.5 : 0.0;
        __syncthreads();
        if (joined) {
            for (int s = hi - 1; s >= 0; --s) {
                int v = i;
                for (int k = 0; k < s; ++k) v = parent(v);
                cov_cross_step<D>(Ho + v * DD, Kb, lane, r, c, ent);
            }
            if (hj > 0) {   // Sigma_ia -> Sigma_ai, then down to j: Sigma_ji
                const double x = ent ? Kb[c * D + r] : 0.0;
                __syncthreads();
                if (ent) Kb[lane] = x;
                __syncthreads();
                for (int s = hj - 1; s >= 0; --s) {
                    int v = j;
                    for (int k = 0; k < s; ++k) v = parent(v);
                    cov_cross_step<D>(Ho + v * DD, Kb, lane, r, c, ent);
                }
            }
        }
        // Kb: Sigma_ji when the second path was walked, Sigma_ij otherwise
        if (lane < 36) {
            const int rr = lane / 6, cc = lane % 6;
            double x = 0.0;
            if (rr < D && cc < D && !((mk[pi] >> rr) & 1) && !((mk[pj] >> cc) & 1)) {
                const bool transposed = (hj == 0) != (pi == i);   // Kb's rows are not the requested pair's first pose
                x = transposed ? Kb[cc * D + rr] : Kb[rr * D + cc];
            }
            out[p * 36 + lane] = x;
        }
    }
}

}  // namespace
}  // namespace locamd
