// gfx950 (MI355X / CDNA4): marginal pose covariances of FOREST windows of <= 64 poses that share ONE topology (BASELINE config 5: the
// key-frame stars of addPoseEdge + anchor ranges), one WAVE per window, on the elimination schedule the host builds for the solve
// kernels (capi_window.cpp: build_tree_sched; TreeSched in window_kernel.h).
//
// What it computes: DESIGN.md §2 word for word — the chain pass's definition (covariance_kernel.hip), always with 6 x 6 blocks.
// With every node eliminated before its parent the factor has no fill: the only later neighbour of node c is its parent p, so
//   upwards (schedule order, children first):  S_c = H_cc - sum_{k child of c} K_k H_{k,c},  K_c = H_{p,c} S_c^-1;
//   downwards (reverse order, roots first):    Sigma_r = S_r^-1 for a root,  Sigma_c = S_c^-1 + K_c^T Sigma_p K_c otherwise.
// H_{p,c} is the sum over ALL edges on the pair (child, parent): several EdgeSE3, a smoothness range next to an EdgeSE3, either direction.
//
// Mapping (one workgroup of one wave per window):
//   * linearisation: lane = edge, the records of cov_block_device.h in LDS (ranges and priors in chunks of 64, EdgeSE3 in chunks of
//     kFcSe3Chunk = 32: the three kinds of records share one LDS region, which keeps a 64-pose window at 60 KB — two windows per CU);
//   * assembly: lane = entry (r, c), the records of a chunk added in edge order (no atomics, every entry owned by one lane: the same
//     bits on every run): H_vv and H_{parent(v),v} by pose slot (every node has one parent: two blocks per pose);
//   * the two sweeps node after node in schedule order (cov_eliminate_block / cov_back_substitute_block): a parent collects from its
//     children in schedule order.
// Every window of the batch has the schedule's counts and index tables (the host compared them), so the loops below are uniform.
#include "cov_block_device.h"

#include <atomic>

namespace locamd {

namespace {

extern __shared__ double fclds[];

constexpr int kFcSe3Chunk = 32;   // EdgeSE3 factors linearised per pass

// LDS layout of one window (offsets in doubles; the int tables follow the doubles)
struct ForestCovLayout {
    int hd, ho, kb, dg, rec, ints, ei, mk, nd, ps;
    size_t bytes;
};
__host__ __device__ inline ForestCovLayout forest_cov_layout(int nv, bool priors, bool se3) {
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

// The block steps below are the chain pass's (covariance_kernel.hip: its forward / backward loops and its store) with "parent" in place of
// "next pose"; they stay a copy because the chain kernel's code changes when its loops are moved into functions.
// Eliminates node i (pose slot i of the window's LDS blocks: Hd = diagonal blocks, Ho = the blocks H_{parent,node} with the parent's rows, dg =
// diag(H)): Hd[i] holds S_i, the node's diagonal block minus its children's shares.  Every lane factors S_i (Cholesky, pivots checked) in its
// registers; S_i^-1 = L^-T L^-1 replaces S_i.  With a parent (slot ip): K_i = H_{ip,i} S_i^-1 replaces Ho[i] and Hd[ip] loses K_i H_{i,ip}.
// Kb: one D x D exchange block.  ok: cleared by a pivot that is not finite, not positive or at most kCovRelPivot of its coordinate's
// diagonal entry of H.
template <int D>
__device__ __forceinline__ void cov_eliminate_block(double* Hd, double* Ho, const double* dg, double* Kb, int i, bool has_parent, int ip, int lane, int r, int c, bool ent, bool& ok) {
    constexpr int DD = D * D;
    double A[D][D];
#pragma unroll
    for (int cc = 0; cc < D; ++cc)
#pragma unroll
        for (int rr = cc; rr < D; ++rr) A[rr][cc] = Hd[i * DD + rr * D + cc];
    double ig[D];
#pragma unroll
    for (int j = 0; j < D; ++j) {
        // numerically singular: the pivot is at most kCovRelPivot of the coordinate's diagonal entry of H (a rank-deficient H leaves pivots of
        // rounding size, 1e-16 .. 1e-14 of it, and of either sign: the absolute test alone would pass half of them); NaN fails as well
        ok = ok && A[j][j] > kCovRelPivot * dg[i * D + j];
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
    double Li[D][D];
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

template <int JAC>
__global__ void __launch_bounds__(64) forest_covariance_kernel(const WindowArgs a, const TreeSched ts, double* cov, int32_t* mask, int32_t* status) {
    constexpr int D = 6, DD = 36, RS = 13;
    const int lane = threadIdx.x;
    const long long inst = blockIdx.x;
    const WindowCaps& cp = a.caps;
    const int nvm = cp.nv_max;
    const int nv = ts.nv, nr = ts.nr, np = ts.np, ns = ts.ns;
    const ForestCovLayout lay = forest_cov_layout(nv, np > 0, ns > 0);
    double* Hd = fclds + lay.hd;
    double* Ho = fclds + lay.ho;
    double* Kb = fclds + lay.kb;
    double* dg = fclds + lay.dg;
    double* rec = fclds + lay.rec;
    int* ib = reinterpret_cast<int*>(fclds + lay.ints);
    int* ei = ib + lay.ei;
    int* mk = ib + lay.mk;
    int* nd = ib + lay.nd;
    int* ps = ib + lay.ps;
    const double* P = a.poses + (size_t)inst * nvm * 12;
    const int r = lane / D, c = lane % D;
    const bool ent = lane < DD;
    for (int k = lane; k < nv * DD; k += 64) { Hd[k] = 0.0; Ho[k] = 0.0; }
    if (lane < nv) { nd[lane] = ts.node[lane]; ps[lane] = ts.w_par[lane]; }

    // ---- linearisation + assembly --------------------------------------------------------------------------------------------------
    for (int e0 = 0; e0 < nr; e0 += kCovChunk) {
        __syncthreads();
        const int e = e0 + lane;
        if (e < nr) {
            const double* val = a.r_val + ((size_t)inst * cp.nr_max + e) * 5;
            const int v0 = ts.r_idx[2 * e], v1 = ts.r_idx[2 * e + 1];
            double X0[12], X1[12], p1[3];
#pragma unroll
            for (int k = 0; k < 12; ++k) X0[k] = P[v0 * 12 + k];
            const int v1c = v1 >= 0 ? v1 : v0;
#pragma unroll
            for (int k = 0; k < 12; ++k) X1[k] = P[v1c * 12 + k];
            if (v1 >= 0) { p1[0] = X1[9]; p1[1] = X1[10]; p1[2] = X1[11]; }
            else { const double* an = a.anchors + (size_t)(-1 - v1) * 3; p1[0] = an[0]; p1[1] = an[1]; p1[2] = an[2]; }
            cov_range_rec<D, JAC>(X0, X1, p1, v1 >= 0, val, rec + lane * RS);
            ei[2 * lane] = v0; ei[2 * lane + 1] = v1;
        }
        __syncthreads();
        if (ent) {
            const int m = min(kCovChunk, nr - e0);
            for (int k = 0; k < m; ++k) {
                const double* q = rec + k * RS;
                const int a0 = ei[2 * k], a1 = ei[2 * k + 1];
                const double w = q[0];
                Hd[a0 * DD + lane] += w * (q[1 + r] * q[1 + c]);
                if (a1 >= 0) {
                    Hd[a1 * DD + lane] += w * (q[1 + D + r] * q[1 + D + c]);
                    if (ps[a0] == a1) Ho[a0 * DD + lane] += w * (q[1 + D + r] * q[1 + c]);   // rows: the parent
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
            cov_prior_block(a.p_val + ((size_t)inst * cp.np_max + e) * 18, P + v * 12, rec + lane * 21);
            ei[lane] = v;
        }
        __syncthreads();
        if (ent) {
            const int m = min(kCovChunk, np - e0);
            for (int k = 0; k < m; ++k) Hd[ei[k] * DD + lane] += rec[k * 21 + LOCAMD_CV_TRI(r, c)];
        }
    }
    for (int e0 = 0; e0 < ns; e0 += kFcSe3Chunk) {
        __syncthreads();
        const int e = e0 + lane;
        if (lane < kFcSe3Chunk && e < ns) {
            const int vi = ts.s_idx[4 * e], vj = ts.s_idx[4 * e + 1];
            double Xi[12], Xj[12], bi[6], bj[6], rterm;
#pragma unroll
            for (int k = 0; k < 12; ++k) { Xi[k] = P[vi * 12 + k]; Xj[k] = P[vj * 12 + k]; }
            double* q = rec + lane * kCovSRec;
            // (the coupling block with the rows of the PARENT: the pose eliminated later)
            chain_se3_terms<true>(Xi, Xj, a.s_val + ((size_t)inst * cp.ns_max + e) * 48, ts.s_idx[4 * e + 2] != 0, ps[vi] == vj, q, q + 21, q + 42, bi, bj, rterm);
            ei[2 * lane] = vi; ei[2 * lane + 1] = vj;
        }
        __syncthreads();
        if (ent) {
            const int m = min(kFcSe3Chunk, ns - e0);
            for (int k = 0; k < m; ++k) {
                const double* q = rec + k * kCovSRec;
                const int vi = ei[2 * k], vj = ei[2 * k + 1];
                Hd[vi * DD + lane] += q[LOCAMD_CV_TRI(r, c)];
                Hd[vj * DD + lane] += q[21 + LOCAMD_CV_TRI(r, c)];
                Ho[(ps[vi] == vj ? vi : vj) * DD + lane] += q[42 + 6 * c + r];
            }
        }
    }
    __syncthreads();
    // ---- excluded coordinates: a diagonal entry exactly 0 (its row and column are 0 as well) ---------------------------------------------
    if (lane < nv) mk[lane] = cov_exclude_zero_diagonal<D>(Hd + lane * DD, dg + lane * D);
    __syncthreads();

    // ---- upwards: S_v, its Cholesky factor, S_v^-1, K_v; the parent's block loses the node's share ----------------------------------------
    bool ok = true;
    for (int k = 0; k < nv; ++k) {
        const int v = nd[k], p = ps[v];
        cov_eliminate_block<D>(Hd, Ho, dg, Kb, v, p >= 0, p >= 0 ? p : v, lane, r, c, ent, ok);
    }
    // ---- downwards: Sigma_v = S_v^-1 + K_v^T Sigma_parent K_v (a root keeps S_v^-1) --------------------------------------------------------
    for (int k = nv - 1; k >= 0; --k) {
        const int v = nd[k], p = ps[v];
        if (p >= 0) cov_back_substitute_block<D>(Hd, Ho, Kb, v, p, lane, r, c, ent);
    }
    cov_store_window<D>(Hd, mk, nv, nvm, ok, lane, inst, cov, mask, status);
}

template <int JAC>
hipError_t launch_forest_cov_t(const WindowArgs& a, const TreeSched& ts, size_t lds, double* cov, int32_t* mask, int32_t* status, hipStream_t stream) {
    static std::atomic<uint64_t> attr_set{0};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const uint64_t bit = 1ull << (dev & 63);
    if (!(attr_set.load(std::memory_order_acquire) & bit)) {
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(&forest_covariance_kernel<JAC>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
        attr_set.fetch_or(bit, std::memory_order_release);
    }
    hipLaunchKernelGGL((forest_covariance_kernel<JAC>), dim3((unsigned)a.B), dim3(64), lds, stream, a, ts, cov, mask, status);
    return hipGetLastError();
}

}  // namespace

size_t window_forest_covariance_lds_bytes(const TreeSched& ts) {
    return forest_cov_layout(ts.nv, ts.np > 0, ts.ns > 0).bytes;
}

hipError_t launch_window_forest_covariance(const WindowArgs& a, const TreeSched& ts, double* cov, int32_t* mask, int32_t* status, hipStream_t stream) {
    if (a.B <= 0) return hipSuccess;
    // (the LDS blocks are indexed by pose slot and the tables by edge number: the schedule must be the batch's own)
    if (ts.nv < 2 || ts.nv > 64 || ts.nv > a.caps.nv_max || ts.nr > a.caps.nr_max || ts.np > a.caps.np_max || ts.ns > a.caps.ns_max) return hipErrorInvalidValue;
    const size_t lds = window_forest_covariance_lds_bytes(ts);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    return a.jacobian ? launch_forest_cov_t<1>(a, ts, lds, cov, mask, status, stream) : launch_forest_cov_t<0>(a, ts, lds, cov, mask, status, stream);
}

}  // namespace locamd
