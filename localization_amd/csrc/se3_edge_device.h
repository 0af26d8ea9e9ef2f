// The 6-DoF factors that are stated once for several kernels: the unary EdgeSE3Prior (prior_terms and the products on its J) and the
// binary EdgeSE3 (chain_se3_terms).  Internal to the including translation unit; every function is inlined and takes poses its caller
// has ALREADY loaded (choosing between two local arrays through a pointer pins both in scratch memory: tree_wave_kernel.hip).  No
// fp-contract pragma of its own: every caller sees these functions under the mode window_device.h leaves behind.
//  * prior_terms: window_kernel.hip (evaluate_edges, both twins), tree_kernel.hip, cov_block_device.h (cov_prior_block, _full).
//    chain_kernel.hip and tree_wave_kernel.hip keep their prior written out: shared, chain_lm_kernel's analytic bits and
//    tree_wave_kernel<1>'s registers and time moved.
//  * chain_se3_terms: chain, forest, wave6 and covariance kernels, the audit.  window_kernel.hip keeps its EdgeSE3 branch written
//    out: shared, 15 of its 24 instantiations moved in scratch.
//  * EdgeSE3Range stays written out in every kernel (the same findings); rho' Omega is info / (1 + chi) in the solve kernels and
//    (1 / (1 + chi)) * info in cov_range_rec — different roundings, both kept.
// (The file keeps the name it had when it held EdgeSE3 alone: bench.py's per-leg source hashes name it.)
// NOT stated here, on purpose: wave6_kernel.hip's w6_edge / w6_prior (different arithmetic: sqrt_and_rsqrt, near roots, fast_rcp,
// mat_to_quat_rsq); the translation-only kernels (wave3, chain3, arrow3, arrow_covariance's 3 x 3 loops), snapshot and fusion; every
// block step and LM loop, the host side and the C ABI.
#pragma once
#include "window_device.h"

namespace locamd {
namespace {

// One unary EdgeSE3Prior at pose X (val: Z^-1 as R(9), t(3)): err = toVectorMQT(Z^-1 X); FULL: J = blockdiag(R_E, Q) (6x6 row-major).
template <bool FULL>
__device__ __forceinline__ void prior_terms(const double* val, const double* X, double* err, double* J) {
    double RE[9], tE[3], q[4];
    mat_mul(val, X, RE);
    mat_vec(val, X + 9, tE);
    tE[0] += val[9]; tE[1] += val[10]; tE[2] += val[11];
    mat_to_quat(RE, q);
    quat_normalize_sign(q);
    err[0] = tE[0]; err[1] = tE[1]; err[2] = tE[2]; err[3] = q[1]; err[4] = q[2]; err[5] = q[3];
    if (FULL) {
#pragma unroll
        for (int i = 0; i < 36; ++i) J[i] = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) J[i * 6 + j] = RE[i * 3 + j];
        quat_right_jac(q, 1.0, J, 6);
    }
}
// chi2 of a prior with the DIAGONAL information W (6); not robust
__device__ __forceinline__ double prior_diag_chi(const double* W, const double* err) {
    double chi = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) chi += err[i] * (W[i] * err[i]);
    return chi;
}
// J^T W J of that prior, lower triangle (21, k = r (r + 1) / 2 + c).  Row i of J touches the columns of its own 3-block only, so entry
// (r, c) is non-zero only inside a diagonal 3-block (IEEE arithmetic cannot drop 0 * x by itself).  The full-W form: prior_full_hessian.
__device__ __forceinline__ void prior_diag_hessian(const double* J, const double* W, double* h) {
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int cc = 0; cc <= r; ++cc) {
            double s = 0.0;
            if ((r < 3) == (cc < 3)) {
#pragma unroll
                for (int i = (r < 3 ? 0 : 3); i < (r < 3 ? 3 : 6); ++i) s += J[i * 6 + r] * W[i] * J[i * 6 + cc];
            }
            h[r * (r + 1) / 2 + cc] = s;
        }
}
// ... and b = J^T (-W e), h[21 .. 26]: both into one record of 27.  h is complete before a caller stores it (window_kernel.hip's record) or
// adds it to a pose's sums (tree_kernel.hip): the same bits either way.  (Full W: window_kernel.hip forms W e for its chi2 and b.)
__device__ __forceinline__ void prior_diag_products(const double* J, const double* W, const double* err, double* h) {
    prior_diag_hessian(J, W, h);
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        double bb = 0.0;
#pragma unroll
        for (int i = (r < 3 ? 0 : 3); i < (r < 3 ? 3 : 6); ++i) bb += J[i * 6 + r] * (-W[i] * err[i]);
        h[21 + r] = bb;
    }
}

// One EdgeSE3 (addPoseEdge / addTwistEdge: localization.cpp:254-290, 438-459, 560-605) between the poses i and j: Jj from E' = E * Delta,
// Ji from E' = A * Delta^-1 * B; WJ = w Omega J, H_ii = J0^T WJ0, H_jj = J1^T WJ1, b = J^T omega_r with omega_r = -w Omega e.  Structure
// (IEEE arithmetic cannot drop 0 * x by itself, so it is spelled out): J1 = [[RE, 0], [0, Q1]]: column c has rows [0,3) if c < 3, else [3,6);
// J0 = [[-A, 2 R A S], [0, Q0]]: column c has rows [0,3) if c < 3, else [0,6).  Returns chi; rterm = the edge's robust cost; FULL: H_ii, H_jj (lower triangles, 21), the off-diagonal block with the
// rows of the LATER pose (36, column-major), b_i, b_j.
// VS: stride of the record's entries in doubles (1: a plain array; 64: one lane's column of an [entry][lane] LDS block — the inverse
// measurement is copied to registers, the information matrix is read where it is used).
template <bool FULL, int VS = 1>
__device__ __forceinline__ double chain_se3_terms(const double* Xi, const double* Xj, const double* val_, bool robust, bool j_is_later,
                                                  double* Hii, double* Hjj, double* Hoff, double* bi_, double* bj_, double& rterm) {
    double val[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) val[k] = val_[VS * k];
    double RB[9], tB[3], dt[3] = {Xj[9] - Xi[9], Xj[10] - Xi[10], Xj[11] - Xi[11]};
    mat_tmul(Xi, Xj, RB);
    mat_tvec(Xi, dt, tB);
    double RE[9], tE[3];
    mat_mul(val, RB, RE);
    mat_vec(val, tB, tE);
    tE[0] += val[9]; tE[1] += val[10]; tE[2] += val[11];
    double qE[4];
    mat_to_quat(RE, qE);
    quat_normalize_sign(qE);
    const double err[6] = {tE[0], tE[1], tE[2], qE[1], qE[2], qE[3]};
    const double* Om_ = val_ + VS * 12;
#define Om(k) Om_[VS * (k)]
    double Oe[6];
    double chi = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double r = 0.0;
#pragma unroll
        for (int j = 0; j < 6; ++j) r += Om(i * 6 + j) * err[j];
        Oe[i] = r;
        chi += err[i] * r;
    }
    const double aux = 1.0 + chi;
    rterm = robust ? fast_log_ge1(aux) : chi;
    if (FULL) {
        const double w = robust ? 1.0 / aux : 1.0;
        double J0[36], J1[36];
#pragma unroll
        for (int i = 0; i < 36; ++i) { J0[i] = 0.0; J1[i] = 0.0; }
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) J1[i * 6 + j] = RE[i * 3 + j];
        quat_right_jac(qE, 1.0, J1, 6);
        const double S[9] = {0, -tB[2], tB[1], tB[2], 0, -tB[0], -tB[1], tB[0], 0};
        double RAS[9];
        mat_mul(val, S, RAS);
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) { J0[i * 6 + j] = -val[i * 3 + j]; J0[i * 6 + 3 + j] = 2.0 * RAS[i * 3 + j]; }
        double qA[4], qB[4], qAB[4];
        mat_to_quat(val, qA);
        mat_to_quat(RB, qB);
        quat_mul(qA, qB, qAB);
        const double sg = qAB[0] < 0 ? -1.0 : 1.0;
        const double nrm = 1.0 / sqrt(qAB[0] * qAB[0] + qAB[1] * qAB[1] + qAB[2] * qAB[2] + qAB[3] * qAB[3]);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            double ek[4] = {0, 0, 0, 0}, r1[4], r2[4];
            ek[1 + k] = 1.0;
            quat_mul(qA, ek, r1);
            quat_mul(r1, qB, r2);
#pragma unroll
            for (int i = 0; i < 3; ++i) J0[(3 + i) * 6 + 3 + k] = -sg * nrm * r2[1 + i];
        }
#define LOCAMD_J1_LO(c) ((c) < 3 ? 0 : 3)
#define LOCAMD_J1_HI(c) ((c) < 3 ? 3 : 6)
#define LOCAMD_J0_HI(c) ((c) < 3 ? 3 : 6)
        double WJ[36];
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int cc = 0; cc < 6; ++cc) {
                double s0 = 0.0;
#pragma unroll
                for (int j = 0; j < LOCAMD_J0_HI(cc); ++j) s0 += Om(i * 6 + j) * J0[j * 6 + cc];
                WJ[i * 6 + cc] = w * s0;
            }
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int cc = 0; cc <= r; ++cc) {
                double h = 0.0;
#pragma unroll
                for (int i = 0; i < LOCAMD_J0_HI(r); ++i) h += J0[i * 6 + r] * WJ[i * 6 + cc];
                Hii[r * (r + 1) / 2 + cc] = h;
            }
        if (j_is_later) {
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int cc = 0; cc < 6; ++cc) {
                    double h = 0.0;
#pragma unroll
                    for (int i = LOCAMD_J1_LO(r); i < LOCAMD_J1_HI(r); ++i) h += J1[i * 6 + r] * WJ[i * 6 + cc];
                    Hoff[6 * cc + r] = h;
                }
        }
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int cc = 0; cc < 6; ++cc) {
                double s1 = 0.0;
#pragma unroll
                for (int j = LOCAMD_J1_LO(cc); j < LOCAMD_J1_HI(cc); ++j) s1 += Om(i * 6 + j) * J1[j * 6 + cc];
                WJ[i * 6 + cc] = w * s1;
            }
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int cc = 0; cc <= r; ++cc) {
                double h = 0.0;
#pragma unroll
                for (int i = LOCAMD_J1_LO(r); i < LOCAMD_J1_HI(r); ++i) h += J1[i * 6 + r] * WJ[i * 6 + cc];
                Hjj[r * (r + 1) / 2 + cc] = h;
            }
        if (!j_is_later) {
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int cc = 0; cc < 6; ++cc) {
                    double h = 0.0;
#pragma unroll
                    for (int i = 0; i < LOCAMD_J0_HI(r); ++i) h += J0[i * 6 + r] * WJ[i * 6 + cc];
                    Hoff[6 * cc + r] = h;
                }
        }
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            double bi = 0.0, bj = 0.0;
#pragma unroll
            for (int i = 0; i < LOCAMD_J0_HI(r); ++i) bi += J0[i * 6 + r] * (-w * Oe[i]);
#pragma unroll
            for (int i = LOCAMD_J1_LO(r); i < LOCAMD_J1_HI(r); ++i) bj += J1[i * 6 + r] * (-w * Oe[i]);
            bi_[r] = bi;
            bj_[r] = bj;
        }
#undef LOCAMD_J1_LO
#undef LOCAMD_J1_HI
#undef LOCAMD_J0_HI
    }
#undef Om
    return chi;
}

}  // namespace
}  // namespace locamd
