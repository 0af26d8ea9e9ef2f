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
//   * the two sweeps node after node in schedule order (cov_eliminate_block / cov_back_substitute_block of cov_block_device.h, the
//     chain pass's steps with "parent" in place of "next pose"): a parent collects from its children in schedule order.
// Every window of the batch has the schedule's counts and index tables (the host compared them), so the loops below are uniform.
//
// Windows of DIFFERING topologies (option "forest_groups_covariance") run the same kernel with one schedule per group of windows of one
// topology: SCHED = TreeGroups, wave_sched of tree_sched_device.h, instantiated in forest_covariance_groups_kernel.hip.  nv, nr, np, ns and the
// LDS offsets are then per-wave values (uniform over the wave: one workgroup of one wave per window), everything else is shared word for word.
#include "cov_block_device.h"
#include "window_kernel.h"
#include "tree_sched_device.h"

namespace locamd {

namespace {

extern __shared__ double fclds[];

template <int JAC, bool JOINT, class SCHED>
__global__ void __launch_bounds__(64) forest_covariance_kernel(const WindowArgs a, const SCHED sched, double* cov, int32_t* mask, int32_t* status, const CovPairs pp) {
    constexpr int D = 6, DD = 36, RS = 13;
    const int lane = threadIdx.x;
    const long long inst = blockIdx.x;
    const TreeSched& ts = wave_sched(sched, a, inst);
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
            cov_range_edge<D, JAC>(P, a.anchors, v0, v1, val, rec + lane * RS);
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
    // ---- joint calls: the cross blocks through the lowest common ancestor, on the parent table in LDS ----------------------------------------
    if (JOINT) cov_store_cross<D>(Hd, Ho, Kb, mk, nv, ok, lane, r, c, ent, inst, pp, [ps](int v) { return ps[v]; });
}

template <int JAC, bool JOINT, class SCHED>
hipError_t launch_forest_cov_j(const WindowArgs& a, const SCHED& s, size_t lds, double* cov, int32_t* mask, int32_t* status, const CovPairs& pp, hipStream_t stream) {
    const hipError_t e = allow_dynamic_lds<&forest_covariance_kernel<JAC, JOINT, SCHED>>((int)kCovMaxLds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((forest_covariance_kernel<JAC, JOINT, SCHED>), dim3((unsigned)a.B), dim3(64), lds, stream, a, s, cov, mask, status, pp);
    return hipGetLastError();
}
template <class SCHED>
hipError_t launch_forest_cov(const WindowArgs& a, const SCHED& s, size_t lds, double* cov, int32_t* mask, int32_t* status, const CovPairs& pp, hipStream_t stream) {
    if (a.jacobian) return pp.cross ? launch_forest_cov_j<1, true>(a, s, lds, cov, mask, status, pp, stream) : launch_forest_cov_j<1, false>(a, s, lds, cov, mask, status, pp, stream);
    return pp.cross ? launch_forest_cov_j<0, true>(a, s, lds, cov, mask, status, pp, stream) : launch_forest_cov_j<0, false>(a, s, lds, cov, mask, status, pp, stream);
}

}  // namespace

// (one instantiation family per translation unit, as tree_wave_kernel.hip's: forest_covariance_groups_kernel.hip includes this file for
//  SCHED = TreeGroups, so that the four TreeSched kernels stay alone in their module and keep their machine code)
#ifndef LOCAMD_FOREST_COV_GROUPS
size_t window_forest_covariance_lds_bytes(const TreeSched& ts) { return forest_cov_layout(ts.nv, ts.np > 0, ts.ns > 0).bytes; }

hipError_t launch_window_forest_covariance(const WindowArgs& a, const TreeSched& ts, double* cov, int32_t* mask, int32_t* status, const CovPairs& pp, hipStream_t stream) {
    if (a.B <= 0) return hipSuccess;
    // (the LDS blocks are indexed by pose slot and the tables by edge number: the schedule must be the batch's own)
    if (!forest_cov_sizes_ok(ts, a.caps)) return hipErrorInvalidValue;
    return launch_forest_cov(a, ts, forest_cov_layout(ts.nv, ts.np > 0, ts.ns > 0).bytes, cov, mask, status, pp, stream);
}
#else
// Every group's sizes are held to the one-topology launcher's bounds on the host's copy of the headers; the launch's dynamic LDS is the
// largest group's layout and every wave uses its own group's offsets inside it.  KNOWN LIMIT: one 64-pose group in the batch puts every
// window of the launch at that group's 60 KB (two windows per CU), whatever its own length.
hipError_t launch_window_forest_covariance_groups(const WindowArgs& a, const TreeGroups& g, const int32_t* host_hdr, double* cov, int32_t* mask, int32_t* status,
                                                  const CovPairs& pp, hipStream_t stream) {
    if (a.B <= 0) return hipSuccess;
    if (!g.hdr || !g.sched_of || !g.tables) return hipErrorInvalidValue;
    const size_t lds = forest_cov_groups_lds_bytes(host_hdr, g.n_groups, a.caps);
    if (lds == 0) return hipErrorInvalidValue;
    return launch_forest_cov(a, g, lds, cov, mask, status, pp, stream);
}
#endif

}  // namespace locamd
