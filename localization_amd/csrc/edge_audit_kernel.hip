// gfx950 (MI355X / CDNA4): the per-edge chi2 audit of a batch of windows and the reference's outlier-range removal (loc_window_edge_chi2_host,
// loc_window_edge_chi2_resident, loc_window_prune_resident; DESIGN.md §2, "Edge audit and outlier removal") — the block Localization::solve()
// keeps after optimizer.optimize() (localization.cpp:172-181): with more than 100 active edges, every range edge (dimension 1) whose chi2()
// exceeds 2.0 goes to level 1 and is left out of every later initializeOptimization().  Here, for window b at x = a.poses:
//   chi2 of a row = BaseEdge::chi2() = e^T Omega e, not robustified, of every structure's three row kinds:
//     range   e = ||X0 o0 - p1|| - meas (p1 = X1 o1, anchor + o1, or either without o1), chi2 = e (info e) — ONE arithmetic form whatever the
//             handle's Jacobian mode: range_error_plain / perturbed_point_plain, the plain-CPU operation order of the numeric solves;
//     prior   e = toVectorMQT(Z^-1 X), W = diag(p_val[12..17]) or the row of the handle's table of full matrices;
//     EdgeSE3 e = toVectorMQT(Z^-1 Xi^-1 Xj), Omega = the 6 x 6 of s_val (chain_se3_terms: the solve kernels' own statement); `robust` does not enter;
//   total = the sum over all rows; active = (range rows with information != 0) + np + ns: level 1 IS information exactly 0.0;
//   prune: if active > min_edges, every range row with information != 0 and chi2 > chi2_max (both strict; NaN compares false and stays) gets
//     removed = 1 and r_val[.][1] = 0.0.  The decision uses the count from BEFORE any store of this launch.
//
// Mapping: one wave per window, rows over lanes, 64 rows at a time.  r_val rows are 40 bytes: a chunk's 320 doubles are staged through LDS with
// unit-stride loads (lane + 64 j) and read back row-wise (stride 5 doubles: odd, no bank conflicts); prior and EdgeSE3 rows (144 / 384 bytes,
// each lane consumes whole cache lines) and the gathered poses come straight from memory.  No scratch.  Every sum runs per lane in row order
// (ranges, priors, EdgeSE3) and ends in wave_sum's fixed tree: the same bits on every run and for every position of a window in the batch.
// The zeroed information is an ordinary vector store from the lane that owns the row.
#include "se3_edge_device.h"
#include "window_kernel.h"

namespace locamd {

namespace {

constexpr int kAuditChunk = 64;   // rows per pass (one per lane)

// e = toVectorMQT(Z^-1 X) of a unary EdgeSE3Prior: the operations of se3_edge_device.h's prior_terms, val = Z^-1 as R(9), t(3)
__device__ __forceinline__ void audit_prior_error(const double* val, const double* X, double* err) {
    double RE[9], tE[3], q[4];
    mat_mul(val, X, RE);
    mat_vec(val, X + 9, tE);
    mat_to_quat(RE, q);
    quat_normalize_sign(q);
    err[0] = tE[0] + val[9]; err[1] = tE[1] + val[10]; err[2] = tE[2] + val[11];
    err[3] = q[1]; err[4] = q[2]; err[5] = q[3];
}

// OFF1: a.r_off1 holds endpoint-1 lever arms; PINFO: a.p_info holds the priors' full matrices; PRUNE: the removal (ranges alone: the other
// rows enter through their counts) — otherwise the audit of every row
template <bool OFF1, bool PINFO, bool PRUNE>
__global__ void __launch_bounds__(64) edge_audit_kernel(const WindowArgs a, const EdgeAudit x) {
    __shared__ double rv[kAuditChunk * 5];
    const int lane = threadIdx.x;
    const long long inst = blockIdx.x;
    const WindowCaps& cp = a.caps;
    const int nr = a.counts[inst * 4 + 1], np = a.counts[inst * 4 + 2], ns = a.counts[inst * 4 + 3];
    const double* P = a.poses + (size_t)inst * cp.nv_max * 12;
    const double* RV = a.r_val + (size_t)inst * cp.nr_max * 5;
    const int32_t* RI = a.r_idx + (size_t)inst * cp.nr_max * 2;

    // ---- prune: the window's active count, before anything is written ----------------------------------------------------------------------
    int active = np + ns;
    if (PRUNE) {
        for (int e0 = 0; e0 < nr; e0 += kAuditChunk) {
            const int e = e0 + lane;
            active += __popcll(__ballot(e < nr && RV[(size_t)e * 5 + 1] != 0.0));
        }
    }
    const bool prune_on = PRUNE && active > x.min_edges;

    // ---- range rows (slots nr .. nr_max - 1: zeros) -------------------------------------------------------------------------------------------
    double tsum = 0.0;
    int n_removed = 0;
    for (int e0 = 0; e0 < cp.nr_max; e0 += kAuditChunk) {
        __syncthreads();
        if (e0 < nr) {
            const int lim = (min(nr, e0 + kAuditChunk) - e0) * 5;
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                const int k = lane + 64 * j;
                if (k < lim) rv[k] = RV[(size_t)e0 * 5 + k];
            }
        }
        __syncthreads();
        const int e = e0 + lane;
        double chi = 0.0;
        bool live = false, rm = false;
        if (e < nr) {
            const double* val = rv + lane * 5;
            const int v0 = RI[e * 2], v1 = RI[e * 2 + 1];
            const double meas = val[0], info = val[1];
            const double off[3] = {val[2], val[3], val[4]};
            const double* X0 = P + v0 * 12;
            double p1[3];
            if (v1 >= 0) { p1[0] = P[v1 * 12 + 9]; p1[1] = P[v1 * 12 + 10]; p1[2] = P[v1 * 12 + 11]; }
            else { const double* an = a.anchors + (size_t)(-1 - v1) * 3; p1[0] = an[0]; p1[1] = an[1]; p1[2] = an[2]; }
            if (OFF1) {   // (X1 * O1).t; a fixed vertex has the identity rotation: anchor + o1 (evaluate_edges' statement)
                const double* o1 = a.r_off1 + ((size_t)inst * cp.nr_max + e) * 3;
                const double off1[3] = {o1[0], o1[1], o1[2]};
                if (v1 >= 0) perturbed_point_plain<0>(P + v1 * 12, P + v1 * 12 + 9, off1, 0.0, p1);
                else { p1[0] = off1[0] + p1[0]; p1[1] = off1[1] + p1[1]; p1[2] = off1[2] + p1[2]; }
            }
            const double err = range_error_plain(X0, X0 + 9, off, p1, meas);
            chi = err * (info * err);
            live = info != 0.0;
            rm = prune_on && live && chi > x.chi2_max;
        }
        if (PRUNE) {
            if (rm) x.prune_r_val[((size_t)inst * cp.nr_max + e) * 5 + 1] = 0.0;
            if (x.removed && e < cp.nr_max) x.removed[(size_t)inst * cp.nr_max + e] = rm ? 1 : 0;
            n_removed += __popcll(__ballot(rm));
        } else {
            active += __popcll(__ballot(live));
            tsum += chi;
            if (x.r_chi2 && e < cp.nr_max) x.r_chi2[(size_t)inst * cp.nr_max + e] = chi;
        }
    }
    if (PRUNE) {
        if (lane == 0 && x.n_removed) x.n_removed[inst] = n_removed;
        return;
    }

    // ---- prior rows ----------------------------------------------------------------------------------------------------------------------
    for (int e0 = 0; e0 < cp.np_max; e0 += kAuditChunk) {
        const int e = e0 + lane;
        double chi = 0.0;
        if (e < np) {
            const double* val = a.p_val + ((size_t)inst * cp.np_max + e) * 18;
            double err[6];
            audit_prior_error(val, P + a.p_idx[(size_t)inst * cp.np_max + e] * 12, err);
            if (PINFO) {
                const double* W = a.p_info + ((size_t)inst * cp.np_max + e) * 36;
#pragma unroll
                for (int i = 0; i < 6; ++i) {
                    double r = 0.0;
#pragma unroll
                    for (int j = 0; j < 6; ++j) r += W[i * 6 + j] * err[j];
                    chi += err[i] * r;
                }
            } else {
#pragma unroll
                for (int i = 0; i < 6; ++i) chi += err[i] * (val[12 + i] * err[i]);
            }
        }
        tsum += chi;
        if (x.p_chi2 && e < cp.np_max) x.p_chi2[(size_t)inst * cp.np_max + e] = chi;
    }

    // ---- EdgeSE3 rows ----------------------------------------------------------------------------------------------------------------------
    for (int e0 = 0; e0 < cp.ns_max; e0 += kAuditChunk) {
        const int e = e0 + lane;
        double chi = 0.0;
        if (e < ns) {
            const int32_t* ix = a.s_idx + ((size_t)inst * cp.ns_max + e) * 4;
            double rterm;
            chi = chain_se3_terms<false>(P + ix[0] * 12, P + ix[1] * 12, a.s_val + ((size_t)inst * cp.ns_max + e) * 48, false, false,
                                         nullptr, nullptr, nullptr, nullptr, nullptr, rterm);
        }
        tsum += chi;
        if (x.s_chi2 && e < cp.ns_max) x.s_chi2[(size_t)inst * cp.ns_max + e] = chi;
    }

    const double total = wave_sum(tsum);
    if (lane == 0) {
        if (x.total) x.total[inst] = total;
        if (x.active) x.active[inst] = active;
    }
}

template <bool OFF1, bool PINFO, bool PRUNE>
hipError_t launch_audit_t(const WindowArgs& a, const EdgeAudit& x, hipStream_t stream) {
    hipLaunchKernelGGL((edge_audit_kernel<OFF1, PINFO, PRUNE>), dim3((unsigned)a.B), dim3(64), 0, stream, a, x);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_window_edge_audit(const WindowArgs& a, const EdgeAudit& x, hipStream_t stream) {
    if (a.B <= 0) return hipSuccess;
    if (x.prune_r_val) {   // (the removal reads no prior: one twin per lever-arm state)
        if (x.prune_r_val != a.r_val) return hipErrorInvalidValue;
        return a.r_off1 ? launch_audit_t<true, false, true>(a, x, stream) : launch_audit_t<false, false, true>(a, x, stream);
    }
    if (a.r_off1) return a.p_info ? launch_audit_t<true, true, false>(a, x, stream) : launch_audit_t<true, false, false>(a, x, stream);
    return a.p_info ? launch_audit_t<false, true, false>(a, x, stream) : launch_audit_t<false, false, false>(a, x, stream);
}

}  // namespace locamd
