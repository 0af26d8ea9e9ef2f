// gfx950 (MI355X / CDNA4): marginal pose covariances of CHAIN windows of <= 64 poses, one WAVE per window.
//
// What it computes: for a window with estimate x (the poses in WindowArgs::poses — the solve's output),
//   H = sum_e J_e^T (rho'_e Omega_e) J_e  at x, no LM damping,
// rho'_e = 1 / (1 + chi2_e) on every range edge and on every EdgeSE3 whose robust flag is set (g2o's robustInformation without rho''),
// priors plain; range Jacobians as the handle's mode says (g2o central differences, delta = 1e-9: range_jac_numeric; or analytic), the
// prior and EdgeSE3 ones analytic as in the solve kernels.  Coordinates: g2o VertexSE3's minimal increment [dt (body frame), dq_xyz]
// applied as x * fromVectorMQT(d).  Output per pose slot v: Sigma_v = [H^-1]_vv (6x6, row-major).
// Unconstrained coordinates (a diagonal entry of H exactly 0.0 — H is a sum of J^T W J with W > 0, so its row and column are 0) are
// excluded: the diagonal is taken as 1 in the factorisation, the output rows / columns are 0 and the coordinate's bit is set in the
// pose's mask (bits 0-5: tx ty tz qx qy qz).  A window whose factorisation meets a pivot that fails window_kernel.hip's test (its
// reciprocal square root is NaN / inf: not finite or <= 0) or that is at most 1e-11 of its coordinate's diagonal entry of H (numerically
// singular: a rank-deficient H) gets status LOC_ERR_SINGULAR and NaN in every block.
//
// Mapping (one workgroup of one wave per window):
//   * linearisation: lane = edge (chunks of 64), the edge's Jacobian blocks / its share of H into a record in LDS; the shared device
//     helpers do the work (range_jac_numeric: window_device.h, chain_se3_terms<true>: se3_edge_device.h);
//   * assembly: lane = entry (r, c) of a D x D block, the records of a chunk added in edge order (no atomics: every entry is owned by one
//     lane, so the result is the same bits on every run): H_ii and H_{i+1,i} in LDS (64 x 2 x 36 doubles = 36 KB for 64 poses);
//   * block-tridiagonal factorisation, pose after pose: S_0 = H_00, K_i = H_{i+1,i} S_i^-1, S_{i+1} = H_{i+1,i+1} - K_i H_{i,i+1}; every
//     lane factors S_i (Cholesky, pivots checked) in its registers and keeps entry (r, c) of S_i^-1 = L^-T L^-1 (cov_eliminate_block);
//   * selected inversion, backwards: Sigma_{n-1} = S_{n-1}^-1, Sigma_i = S_i^-1 + K_i^T Sigma_{i+1} K_i (lane = entry; cov_back_substitute_block).
// D = 3 for translation-only batches (capi_window.cpp: translation_only — 3x3 blocks, the rotation bits always set), D = 6 otherwise.
// PINFO (D = 3 only): the priors' information is the dense 3 x 3 block of their row of a.p_info (a translation-only table, option
// "prior_information_structured") in the place of p_val's diagonal; the exclusion rule and the pivot tests see whatever diagonal results.
#include "cov_block_device.h"
#include "window_kernel.h"

namespace locamd {

namespace {

extern __shared__ double cvlds[];

template <int D, int JAC, bool JOINT, bool PINFO = false>
__global__ void __launch_bounds__(64) covariance_kernel(const WindowArgs a, int nvl, bool priors, bool se3, double* cov, int32_t* mask, int32_t* status, const CovPairs pp) {
    constexpr int DD = D * D;
    constexpr int RS = 1 + 2 * D;
    const int lane = threadIdx.x;
    const long long inst = blockIdx.x;
    const WindowCaps& cp = a.caps;
    const int nvm = cp.nv_max;
    const CovLayout lay = cov_layout(nvl, D, priors, se3);
    double* Hd = cvlds + lay.hd;
    double* Ho = cvlds + lay.ho;
    double* Kb = cvlds + lay.kb;
    double* dg = cvlds + lay.dg;
    double* rrec = cvlds + lay.rrec;
    double* prec = cvlds + lay.prec;
    double* srec = cvlds + lay.srec;
    int* ib = reinterpret_cast<int*>(cvlds + lay.ints);
    int* ri = ib + lay.ri;
    int* pi = ib + lay.pi;
    int* si = ib + lay.si;
    int* mk = ib + lay.mk;
    const int nv = a.counts[inst * 4 + 0], nr = a.counts[inst * 4 + 1], np = a.counts[inst * 4 + 2], ns = se3 ? a.counts[inst * 4 + 3] : 0;
    const double* P = a.poses + (size_t)inst * nvm * 12;
    const int r = lane / D, c = lane % D;
    const bool ent = lane < DD;
    for (int k = lane; k < nv * DD; k += 64) { Hd[k] = 0.0; Ho[k] = 0.0; }

    // ---- linearisation + assembly --------------------------------------------------------------------------------------------------
    for (int e0 = 0; e0 < nr; e0 += kCovChunk) {
        __syncthreads();
        const int e = e0 + lane;
        if (e < nr) {
            const int32_t* ix = a.r_idx + ((size_t)inst * cp.nr_max + e) * 2;
            const double* val = a.r_val + ((size_t)inst * cp.nr_max + e) * 5;
            const int v0 = ix[0], v1 = ix[1];
            // (cov_range_edge's fetch, written out: through the helper covariance_kernel<3, 0> is allocated 78 VGPRs, not 80 — DESIGN.md §4)
            double X0[12], X1[12], p1[3];
#pragma unroll
            for (int k = 0; k < 12; ++k) X0[k] = P[v0 * 12 + k];
            const int v1c = v1 >= 0 ? v1 : v0;
#pragma unroll
            for (int k = 0; k < 12; ++k) X1[k] = P[v1c * 12 + k];
            if (v1 >= 0) { p1[0] = X1[9]; p1[1] = X1[10]; p1[2] = X1[11]; }
            else { const double* an = a.anchors + (size_t)(-1 - v1) * 3; p1[0] = an[0]; p1[1] = an[1]; p1[2] = an[2]; }
            cov_range_rec<D, JAC>(X0, X1, p1, v1 >= 0, val, rrec + lane * RS);
            ri[2 * lane] = v0; ri[2 * lane + 1] = v1;
        }
        __syncthreads();
        if (ent) {
            const int m = min(kCovChunk, nr - e0);
            for (int k = 0; k < m; ++k) {
                const double* q = rrec + k * RS;
                const int a0 = ri[2 * k], a1 = ri[2 * k + 1];
                const double w = q[0];
                Hd[a0 * DD + lane] += w * (q[1 + r] * q[1 + c]);
                if (a1 >= 0) {
                    Hd[a1 * DD + lane] += w * (q[1 + D + r] * q[1 + D + c]);
                    if (a1 == a0 + 1) Ho[a0 * DD + lane] += w * (q[1 + D + r] * q[1 + c]);   // rows: the later pose
                    else Ho[a1 * DD + lane] += w * (q[1 + r] * q[1 + D + c]);
                }
            }
        }
    }
    for (int e0 = 0; e0 < np; e0 += kCovChunk) {
        __syncthreads();
        const int e = e0 + lane;
        if (e < np) {
            const int v = a.p_idx[(size_t)inst * cp.np_max + e];
            if (PINFO) cov_prior_block3(a.p_val + ((size_t)inst * cp.np_max + e) * 18, a.p_info + ((size_t)inst * cp.np_max + e) * 36, P + v * 12, prec + lane * 21);
            else cov_prior_block(a.p_val + ((size_t)inst * cp.np_max + e) * 18, P + v * 12, prec + lane * 21);
            pi[lane] = v;
        }
        __syncthreads();
        if (ent) {
            const int m = min(kCovChunk, np - e0);
            for (int k = 0; k < m; ++k) Hd[pi[k] * DD + lane] += prec[k * 21 + LOCAMD_CV_TRI(r, c)];
        }
    }
    if (D == 6) {
        for (int e0 = 0; e0 < ns; e0 += kCovChunk) {
            __syncthreads();
            const int e = e0 + lane;
            if (e < ns) {
                const int32_t* ix = a.s_idx + ((size_t)inst * cp.ns_max + e) * 4;
                const int vi = ix[0], vj = ix[1];
                double Xi[12], Xj[12], bi[6], bj[6], rterm;
#pragma unroll
                for (int k = 0; k < 12; ++k) { Xi[k] = P[vi * 12 + k]; Xj[k] = P[vj * 12 + k]; }
                double* q = srec + lane * kCovSRec;
                chain_se3_terms<true>(Xi, Xj, a.s_val + ((size_t)inst * cp.ns_max + e) * 48, ix[2] != 0, vj > vi, q, q + 21, q + 42, bi, bj, rterm);
                si[2 * lane] = vi; si[2 * lane + 1] = vj;
            }
            __syncthreads();
            if (ent) {
                const int m = min(kCovChunk, ns - e0);
                for (int k = 0; k < m; ++k) {
                    const double* q = srec + k * kCovSRec;
                    const int vi = si[2 * k], vj = si[2 * k + 1];
                    Hd[vi * DD + lane] += q[LOCAMD_CV_TRI(r, c)];
                    Hd[vj * DD + lane] += q[21 + LOCAMD_CV_TRI(r, c)];
                    Ho[min(vi, vj) * DD + lane] += q[42 + 6 * c + r];
                }
            }
        }
    }
    __syncthreads();
    // ---- excluded coordinates: a diagonal entry exactly 0 (its row and column are 0 as well) ---------------------------------------------
    if (lane < nv) mk[lane] = cov_exclude_zero_diagonal<D>(Hd + lane * DD, dg + lane * D);
    __syncthreads();

    // ---- forward: S_i, its Cholesky factor, S_i^-1, K_i; backward: Sigma_i = S_i^-1 + K_i^T Sigma_{i+1} K_i (the parent of pose i is pose i + 1) ----
    bool ok = true;
    for (int i = 0; i < nv; ++i) cov_eliminate_block<D>(Hd, Ho, dg, Kb, i, i + 1 < nv, i + 1, lane, r, c, ent, ok);
    for (int i = nv - 2; i >= 0; --i) cov_back_substitute_block<D>(Hd, Ho, Kb, i, i + 1, lane, r, c, ent);
    cov_store_window<D>(Hd, mk, nv, nvm, ok, lane, inst, cov, mask, status);
    // ---- joint calls: Sigma_ij = (-K_i^T) .. (-K_{j-1}^T) Sigma_jj for i < j (the chain is the forest with parent = next pose) ------------------
    if (JOINT) cov_store_cross<D>(Hd, Ho, Kb, mk, nv, ok, lane, r, c, ent, inst, pp, [nv](int v) { return v + 1 < nv ? v + 1 : -1; });
}

template <int D, int JAC, bool JOINT, bool PINFO = false>
hipError_t launch_cov_j(const WindowArgs& a, int nvl, bool priors, bool se3, size_t lds, double* cov, int32_t* mask, int32_t* status, const CovPairs& pp, hipStream_t stream) {
    const hipError_t e = allow_dynamic_lds<&covariance_kernel<D, JAC, JOINT, PINFO>>((int)kCovMaxLds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((covariance_kernel<D, JAC, JOINT, PINFO>), dim3((unsigned)a.B), dim3(64), lds, stream, a, nvl, priors, se3, cov, mask, status, pp);
    return hipGetLastError();
}
template <int D, int JAC, bool PINFO = false>
hipError_t launch_cov_t(const WindowArgs& a, int nvl, bool priors, bool se3, size_t lds, double* cov, int32_t* mask, int32_t* status, const CovPairs& pp, hipStream_t stream) {
    return pp.cross ? launch_cov_j<D, JAC, true, PINFO>(a, nvl, priors, se3, lds, cov, mask, status, pp, stream)
                    : launch_cov_j<D, JAC, false, PINFO>(a, nvl, priors, se3, lds, cov, mask, status, pp, stream);
}

}  // namespace

size_t window_covariance_lds_bytes(const WindowCaps& c, bool d3) { return cov_layout(c, d3).bytes; }

hipError_t launch_window_covariance(const WindowArgs& a, bool d3, double* cov, int32_t* mask, int32_t* status, const CovPairs& pp, hipStream_t stream) {
    if (a.B <= 0) return hipSuccess;
    if (a.caps.nv_max > 64) return hipErrorInvalidValue;
    const bool priors = a.caps.np_max > 0, se3 = !d3 && a.caps.ns_max > 0;
    if (!cov_chain_fits(a.caps, d3)) return hipErrorInvalidValue;
    const size_t lds = cov_layout(a.caps, d3).bytes;
    if (a.p_info) {   // (the host admits a table here only where structured_pinfo holds: window_dispatch.cpp, cov_admitted — Chain3 alone)
        if (!d3) return hipErrorInvalidValue;
        return a.jacobian ? launch_cov_t<3, 1, true>(a, a.caps.nv_max, priors, se3, lds, cov, mask, status, pp, stream)
                          : launch_cov_t<3, 0, true>(a, a.caps.nv_max, priors, se3, lds, cov, mask, status, pp, stream);
    }
    if (d3) return a.jacobian ? launch_cov_t<3, 1>(a, a.caps.nv_max, priors, se3, lds, cov, mask, status, pp, stream)
                              : launch_cov_t<3, 0>(a, a.caps.nv_max, priors, se3, lds, cov, mask, status, pp, stream);
    return a.jacobian ? launch_cov_t<6, 1>(a, a.caps.nv_max, priors, se3, lds, cov, mask, status, pp, stream)
                      : launch_cov_t<6, 0>(a, a.caps.nv_max, priors, se3, lds, cov, mask, status, pp, stream);
}

}  // namespace locamd
