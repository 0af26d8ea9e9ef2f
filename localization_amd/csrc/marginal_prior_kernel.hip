// gfx950 (MI355X / CDNA4): the marginal prior a dropped pose leaves on its one neighbour (loc_window_marginal_prior_host; DESIGN.md §2,
// "The marginal prior of a dropped pose"), translation-only windows.  With d = drop[b], m = the one pose that pose-to-pose ranges join to d
// (the host has checked that there is at most one: window_structure.cpp, check_marginal_drop) and x = a.poses:
//   removed factors: every range with d as an endpoint (to anchors; to m, several allowed, in either direction) and every prior on d,
//     linearised at x as the covariance passes do it (rho' = 1 / (1 + chi2) on ranges, the handle's Jacobian mode; priors analytic, not
//     robust, with their full matrix when the handle has a table) — H^r = sum J^T (rho' Omega) J, g^r = sum J^T (rho' Omega) e over (t_d, t_m);
//   excluded coordinates of d (a diagonal entry of H^r_dd exactly 0), the factor of H^r_dd with both pivot tests (cov_chol_inverse);
//   Lambda = H^r_mm - H^r_md (H^r_dd)^-1 H^r_dm (symmetrised), gamma = g^r_m - H^r_md (H^r_dd)^-1 g^r_d;
//   the symmetric eigen-decomposition of Lambda (cyclic Jacobi, a rotation on an exactly-zero entry skipped: structural zeros stay exact),
//     the eigenpairs with lambda_k > 1e-11 lambda_max kept: information = sum lambda_k v_k v_k^T, e0 = sum (v_k^T gamma / lambda_k) v_k;
//   Z^-1 = (I, e0 - t_m): toVectorMQT(Z^-1 X_m) = e0, so EdgeSE3Prior(Z, information) on m has gradient gamma and Hessian Lambda at x.
//
// Mapping: one wave per window.  Lanes scan the edge tables 64 at a time and write the records of d's factors to LDS; lane (r, c) of the
// 6 x 6 matrix over (t_d, t_m) and lanes 36 .. 41 of its gradient then add the chunk's records IN EDGE ORDER (ranges first, then priors):
// the same bits on every run and for every position of the window in the batch.  The 3 x 3 algebra runs in registers with static indices
// (no scratch); lane 0 hands the result over through LDS and the wave stores it.
#include "cov_block_device.h"
#include "window_kernel.h"

namespace locamd {

namespace {

constexpr int kMpRangeRec = 8;    // rho' Omega, J_d (3), J_m (3), error
constexpr int kMpPriorRec = 12;   // W_tt (9, row-major), W_tt e (3)
constexpr int kMpOut = 48 + 6 + 6 + 3;   // prior row, grad, shift, (slot, rank, status)
constexpr int kMpSweeps = 8;      // cyclic Jacobi sweeps of the 3 x 3 (quadratic convergence: five reach rounding level)

// one Jacobi rotation of the symmetric S (both triangles kept) on the entry (P, Q); O: the third index.  V's columns follow.
template <int P, int Q, int O>
__device__ __forceinline__ void mp_jacobi_rotate(double (&S)[3][3], double (&V)[3][3]) {
    const double apq = S[P][Q];
    if (apq == 0.0) return;
    const double theta = (S[Q][Q] - S[P][P]) / (2.0 * apq);
    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c, tau = s / (1.0 + c);
    const double h = t * apq;
    S[P][P] -= h; S[Q][Q] += h;
    S[P][Q] = 0.0; S[Q][P] = 0.0;
    const double g = S[O][P], k = S[O][Q];
    S[O][P] = g - s * (k + g * tau); S[P][O] = S[O][P];
    S[O][Q] = k + s * (g - k * tau); S[Q][O] = S[O][Q];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double vg = V[r][P], vk = V[r][Q];
        V[r][P] = vg - s * (vk + vg * tau);
        V[r][Q] = vk + s * (vg - vk * tau);
    }
}

template <int JAC, bool PINFO>
__global__ void __launch_bounds__(64) marginal_prior_kernel(const WindowArgs a, const int32_t* drop, int32_t* slot, double* prior, double* grad, double* shift,
                                                            int32_t* rank, int32_t* status) {
    __shared__ double rec[kCovChunk * kMpPriorRec];
    __shared__ int kind[kCovChunk];   // != 0: the chunk's edge is a factor of d and has a record
    __shared__ double acc[42];
    __shared__ double outb[kMpOut];
    const int lane = threadIdx.x;
    const long long inst = blockIdx.x;
    const WindowCaps& cp = a.caps;
    const int nr = a.counts[inst * 4 + 1], np = a.counts[inst * 4 + 2];
    const double* P = a.poses + (size_t)inst * cp.nv_max * 12;
    const int d = drop[inst];

    // ---- the neighbour: the host has checked that every pose-to-pose range of d names the same pose -------------------------------------
    int m = -1;
    for (int e = lane; e < nr; e += 64) {
        const int32_t* ix = a.r_idx + ((size_t)inst * cp.nr_max + e) * 2;
        if (ix[1] >= 0) {
            if (ix[0] == d) m = max(m, ix[1]);
            else if (ix[1] == d) m = max(m, ix[0]);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o));

    // ---- linearisation + ordered accumulation: lane (r, c) < 36 of H^r over z = (t_d, t_m), lanes 36 .. 41 of g^r -------------------------------
    const int r = lane < 36 ? lane / 6 : lane - 36, c = lane % 6;
    double sum = 0.0;
    for (int e0 = 0; e0 < nr; e0 += kCovChunk) {
        __syncthreads();
        const int e = e0 + lane;
        int kd = 0;
        if (e < nr) {
            const int32_t* ix = a.r_idx + ((size_t)inst * cp.nr_max + e) * 2;
            const int v0 = ix[0], v1 = ix[1];
            if (v0 == d || v1 == d) {
                // the covariance passes' record (rho' Omega, J of endpoint 0, J of endpoint 1) and the error it weighs the edge with
                double q[7], err;
                cov_range_edge<3, JAC>(P, a.anchors, v0, v1, a.r_val + ((size_t)inst * cp.nr_max + e) * 5, q, &err);
                const bool first = v0 == d;   // J_d = the columns of the endpoint that is d
                double* w = rec + lane * kMpRangeRec;
                w[0] = q[0];
#pragma unroll
                for (int k = 0; k < 3; ++k) { w[1 + k] = first ? q[1 + k] : q[4 + k]; w[4 + k] = first ? q[4 + k] : q[1 + k]; }
                w[7] = err;
                kd = 1;
            }
        }
        kind[lane] = kd;
        __syncthreads();
        if (lane < 42) {
            const int cnt = min(kCovChunk, nr - e0);
            for (int k = 0; k < cnt; ++k) {
                if (!kind[k]) continue;
                const double* q = rec + k * kMpRangeRec;
                // (an anchor range has J_m = 0: cov_range_rec leaves the columns of a fixed endpoint 0)
                if (lane < 36) sum += q[0] * (q[1 + r] * q[1 + c]);
                else sum += q[1 + r] * (q[0] * q[7]);
            }
        }
    }
    for (int e0 = 0; e0 < np; e0 += kCovChunk) {
        __syncthreads();
        const int e = e0 + lane;
        int kd = 0;
        if (e < np && a.p_idx[(size_t)inst * cp.np_max + e] == d) {
            // a translation-only batch (the host's scan): identity rotations, so J = I on the translations and e = t_d + Z^-1.t
            const double* val = a.p_val + ((size_t)inst * cp.np_max + e) * 18;
            const double er[3] = {P[d * 12 + 9] + val[9], P[d * 12 + 10] + val[10], P[d * 12 + 11] + val[11]};
            double* w = rec + lane * kMpPriorRec;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                double we = 0.0;
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const double x = PINFO ? a.p_info[((size_t)inst * cp.np_max + e) * 36 + i * 6 + j] : (i == j ? val[12 + i] : 0.0);
                    w[i * 3 + j] = x;
                    we += x * er[j];
                }
                w[9 + i] = we;
            }
            kd = 1;
        }
        kind[lane] = kd;
        __syncthreads();
        if (lane < 42 && (lane < 36 ? (r < 3 && c < 3) : r < 3)) {
            const int cnt = min(kCovChunk, np - e0);
            for (int k = 0; k < cnt; ++k) {
                if (!kind[k]) continue;
                const double* q = rec + k * kMpPriorRec;
                sum += lane < 36 ? q[r * 3 + c] : q[9 + r];
            }
        }
    }
    if (lane < 42) acc[lane] = sum;
    __syncthreads();

    // ---- the 3 x 3 algebra, every lane alike, static indices -------------------------------------------------------------------------------
    double A[9], Bm[3][3], Cm[3][3], gd[3], gm[3], dg[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) { A[i * 3 + j] = acc[i * 6 + j]; Bm[i][j] = acc[(3 + i) * 6 + j]; Cm[i][j] = acc[(3 + i) * 6 + 3 + j]; }
        gd[i] = acc[36 + i]; gm[i] = acc[39 + i];
    }
    // excluded coordinates of d: a diagonal entry exactly 0 (its row and column, its column of H^r_md and its gradient entry are 0 as well)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (A[k * 3 + k] == 0.0) {
#pragma unroll
            for (int j = 0; j < 3; ++j) { A[k * 3 + j] = 0.0; A[j * 3 + k] = 0.0; Bm[j][k] = 0.0; }
            A[k * 3 + k] = 1.0;
            gd[k] = 0.0;
        }
        dg[k] = A[k * 3 + k];
    }
    bool ok = true;
    double Li[3][3];
    cov_chol_inverse<3>(A, dg, ok, Li);
    double Ai[3][3];   // (H^r_dd)^-1 = L^-T L^-1
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k)
                if (k >= i && k >= j) s = __builtin_fma(Li[k][i], Li[k][j], s);
            Ai[i][j] = s;
        }
    double S[3][3], V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}}, gamma[3], x[3];
    {
        double Y[3][3], Lm[3][3];   // Y = (H^r_dd)^-1 H^r_dm
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) Y[i][j] = Ai[i][0] * Bm[j][0] + Ai[i][1] * Bm[j][1] + Ai[i][2] * Bm[j][2];
            x[i] = Ai[i][0] * gd[0] + Ai[i][1] * gd[1] + Ai[i][2] * gd[2];
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) Lm[i][j] = Cm[i][j] - (Bm[i][0] * Y[0][j] + Bm[i][1] * Y[1][j] + Bm[i][2] * Y[2][j]);
            gamma[i] = gm[i] - (Bm[i][0] * x[0] + Bm[i][1] * x[1] + Bm[i][2] * x[2]);
        }
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) S[i][j] = 0.5 * (Lm[i][j] + Lm[j][i]);
    }
    for (int sweep = 0; sweep < kMpSweeps; ++sweep) {
        mp_jacobi_rotate<0, 1, 2>(S, V);
        mp_jacobi_rotate<0, 2, 1>(S, V);
        mp_jacobi_rotate<1, 2, 0>(S, V);
    }
    const double lmax = fmax(S[0][0], fmax(S[1][1], S[2][2]));
    double info[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, e0[3] = {0, 0, 0};
    int rk = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double lam = S[k][k];
        if (lam > kCovRelPivot * lmax && lam > 0.0) {   // (the pivot rule's constant; NaN fails)
            ++rk;
            const double coef = (V[0][k] * gamma[0] + V[1][k] * gamma[1] + V[2][k] * gamma[2]) / lam;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                e0[i] += coef * V[i][k];
#pragma unroll
                for (int j = 0; j <= i; ++j) info[i][j] += lam * (V[i][k] * V[j][k]);
            }
        }
    }
    // ---- the row: lane 0 hands it over, the wave stores it ----------------------------------------------------------------------------------
    const bool none = m < 0;          // nothing to carry the marginal: slot -1, zeros, identity Z^-1, LOC_OK
    const bool carry = !none && ok;   // a failed pivot (the removed factors do not determine d): the zero row on m — the plain drop
    if (lane == 0) {
        const int mc = none ? 0 : m;
#pragma unroll
        for (int k = 0; k < 9; ++k) outb[k] = (k % 4 == 0) ? 1.0 : 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) outb[9 + k] = none ? 0.0 : (carry ? e0[k] : 0.0) - P[mc * 12 + 9 + k];
#pragma unroll
        for (int k = 0; k < 36; ++k) {
            const int i = k / 6, j = k % 6;
            outb[12 + k] = (carry && i < 3 && j < 3) ? (i >= j ? info[i][j] : info[j][i]) : 0.0;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            outb[48 + k] = carry ? gamma[k] : 0.0; outb[51 + k] = 0.0;
            outb[54 + k] = carry ? e0[k] : 0.0; outb[57 + k] = 0.0;
        }
    }
    __syncthreads();
    if (lane < 48) prior[(size_t)inst * 48 + lane] = outb[lane];
    if (lane < 6) { grad[(size_t)inst * 6 + lane] = outb[48 + lane]; shift[(size_t)inst * 6 + lane] = outb[54 + lane]; }
    if (lane == 0) {
        slot[inst] = none ? -1 : m;
        rank[inst] = carry ? rk : 0;
        status[inst] = (none || ok) ? 0 : -6;   // LOC_OK / LOC_ERR_SINGULAR
    }
}

template <int JAC, bool PINFO>
hipError_t launch_mp_t(const WindowArgs& a, const int32_t* drop, int32_t* slot, double* prior, double* grad, double* shift, int32_t* rank, int32_t* status, hipStream_t stream) {
    hipLaunchKernelGGL((marginal_prior_kernel<JAC, PINFO>), dim3((unsigned)a.B), dim3(64), 0, stream, a, drop, slot, prior, grad, shift, rank, status);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_window_marginal_prior(const WindowArgs& a, const int32_t* drop, int32_t* slot, double* prior, double* grad, double* shift, int32_t* rank, int32_t* status,
                                        hipStream_t stream) {
    if (a.B <= 0) return hipSuccess;
    if (!drop || !slot || !prior || !grad || !shift || !rank || !status) return hipErrorInvalidValue;
    if (a.p_info) return a.jacobian ? launch_mp_t<1, true>(a, drop, slot, prior, grad, shift, rank, status, stream)
                                    : launch_mp_t<0, true>(a, drop, slot, prior, grad, shift, rank, status, stream);
    return a.jacobian ? launch_mp_t<1, false>(a, drop, slot, prior, grad, shift, rank, status, stream)
                      : launch_mp_t<0, false>(a, drop, slot, prior, grad, shift, rank, status, stream);
}

}  // namespace locamd
