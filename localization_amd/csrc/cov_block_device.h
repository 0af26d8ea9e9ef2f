// What the wave-per-window covariance passes do alike (covariance_kernel.hip: chain windows; forest_covariance_kernel.hip: forest windows;
// DESIGN.md §2 / §4): the per-edge records of the linearisation (range, unary prior, the EdgeSE3 record's layout) and the rule for
// excluded coordinates.  (The block factorisation, the K^T Sigma K update and the store are NOT here: moved into functions they change
// the chain kernel's code — DESIGN.md §4 — so each kernel keeps its own.)  Internal to the including translation unit.
#pragma once
#include "se3_edge_device.h"
#include "cov_device.h"

#include <float.h>
#include <math.h>

namespace locamd {
namespace {

constexpr int kCovChunk = 64;   // edges linearised per pass (one per lane)
constexpr int kCovSRec = 21 + 21 + 36;   // EdgeSE3 record: H_ii, H_jj (lower triangles), the coupling block (rows: the later pose, column-major)

#define LOCAMD_CV_TRI(r, c) ((r) >= (c) ? (r) * ((r) + 1) / 2 + (c) : (c) * ((c) + 1) / 2 + (r))

// one unary EdgeSE3Prior at X: its J^T W J (lower triangle, 21) — window_kernel.hip: evaluate_edges, unary priors
__device__ __forceinline__ void cov_prior_block(const double* val, const double* X, double* rec) {
    double RE[9], tE[3], q[4];
    mat_mul(val, X, RE);
    mat_vec(val, X + 9, tE);
    mat_to_quat(RE, q);
    quat_normalize_sign(q);
    double J[36];
#pragma unroll
    for (int i = 0; i < 36; ++i) J[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) J[i * 6 + j] = RE[i * 3 + j];
    quat_right_jac(q, 1.0, J, 6);
    const double* W = val + 12;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int cc = 0; cc <= r; ++cc) {
            double h = 0.0;
            if ((r < 3) == (cc < 3)) {
#pragma unroll
                for (int i = (r < 3 ? 0 : 3); i < (r < 3 ? 3 : 6); ++i) h += J[i * 6 + r] * W[i] * J[i * 6 + cc];
            }
            rec[r * (r + 1) / 2 + cc] = h;
        }
}

// one range edge (no lever arm on endpoint 1): rho' info, J0 (D columns of the pose carrying the lever arm), J1 (D columns of the other pose)
template <int D, int JAC>
__device__ __forceinline__ void cov_range_rec(const double* X0, const double* X1, const double* p1, bool pose1, const double* val, double* rec) {
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
#pragma unroll
    for (int k = 0; k < D; ++k) { rec[1 + k] = J0[k]; rec[1 + D + k] = J1[k]; }
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

}  // namespace
}  // namespace locamd
