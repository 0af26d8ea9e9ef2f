// gfx950 (MI355X / CDNA4): marginal pose covariances of windows of ANY structure and length — what the chain, arrowhead and forest passes
// decline (capi_window.cpp: covariance_kind, option "covariance_general"): chains and forests of more than 64 poses, ragged or mixed batches,
// 6-DoF arrowheads, windows with loops.  One WORKGROUP of 256 threads per window, every window on its own structure.
//
// What it computes: DESIGN.md §2 word for word — the chain pass's definition (covariance_kernel.hip), always with 6 x 6 blocks (a
// translation-only window gets its rotation bits from the exactly-zero-diagonal rule).
//
// Storage: the ENVELOPE (skyline) of the block matrix in the caller's pose order.  first[i] = the smallest slot a pose-to-pose edge joins to
// slot i (i itself without one); row i keeps the blocks (i, first[i]) .. (i, i), rows one after the other (off[] = their prefix sum), in the
// window's slice of an HBM workspace [blocks][36].  The factor of a matrix fills exactly its envelope, so H, its block LDL^T and the
// selected inverse live in the same blocks one after the other.  No reordering: work and memory are what the caller's slot order makes
// them (a star packed leaves-first: 2n - 1 blocks; key-first: n (n + 1) / 2).
//
// With struct(j) = {k > j : first[k] <= j} (the rows that reach column j):
//   forward, column after column:   S_j^-1 (cov_chol_inverse: both pivot tests),  K_kj = H_kj S_j^-1 for k in struct(j),
//                                   H_ik -= K_ij H_jk for the pairs i >= k of struct(j)  (inside the envelope: first[i] <= j < k);
//   backward (selected inversion):  Sigma_ij = -sum_{k in struct(j)} Sigma_ik K_kj for i in struct(j)  (Sigma_ik from the stored lower
//                                   envelope, transposed where i < k),  Sigma_jj = S_j^-1 - sum_{k in struct(j)} K_kj^T Sigma_kj.
// On a chain this is the chain pass's S^-1 + K^T Sigma K.
//
// Mapping: thread = (slot, entry) = (tid / 36, tid % 36): seven 6 x 6 blocks in flight, the last four threads of the workgroup only
// linearise.
//   * profile: first[] by integer LDS atomicMin over the edges (and, in a joint call, over the requested pairs), last[j] = max {k : first[k] <= j} (atomicMax + a running maximum), off[];
//   * linearisation: thread = edge, the records of cov_block_device.h in one LDS region (256 ranges / 128 priors / 64 EdgeSE3 per pass);
//   * assembly: the block ROW decides the owner (row % 7 = slot), every owner walks the chunk's records in edge order and adds its
//     own — no floating-point atomics, every entry summed in edge order whatever the number of threads: the same bits on every run;
//   * a column step: struct(j) as an ordered list (ballot + prefix over rows j + 1 .. last[j]); every thread factors S_j in its registers;
//     the rows of the column and the pairs of its update are spread over the slots, each entry summed by one thread in list order.
//     The column's H_kj are copied to a side array first (the update needs them next to K_kj, which takes their place): a column of
//     at most 69 rows keeps that copy and K_kj in LDS (the record region, free after the assembly), so that its update reads LDS alone
//     and the backward step writes Sigma_kj to its place at once; a taller column goes through the workspace's column array.
// Global memory written by one thread and read by another is always separated by __syncthreads() (one workgroup = one CU: its vector L1
// is shared).
#include "cov_block_device.h"
#include "window_kernel.h"

namespace locamd {

namespace {

extern __shared__ double evlds[];

// struct(j) into list[] in ascending order; returns its size (the same value in every thread).  Barriers inside: call it uniformly.
__device__ __forceinline__ int env_column_rows(int j, const int* first, const int* last, int* list, int* wc, int tid) {
    const int top = last[j];
    int m = 0;
    for (int k0 = j + 1; k0 <= top; k0 += kEvThreads) {
        const int k = k0 + tid;
        const bool in = k <= top && first[k] <= j;
        const unsigned long long b = __ballot(in);
        const int lane = tid & 63, wv = tid >> 6;
        if (lane == 0) wc[wv] = __popcll(b);
        __syncthreads();
        int base = m;
        for (int x = 0; x < wv; ++x) base += wc[x];
        if (in) list[base + __popcll(b & ((1ull << lane) - 1ull))] = k;
        m += wc[0] + wc[1] + wc[2] + wc[3];
        __syncthreads();
    }
    return m;
}

// PINFO: the priors' information matrices are the full rows of a.p_info (loc_window_set_prior_information) — a twin of every variant, so that
// the pass of every other handle is the machine code it was
template <int JAC, bool JOINT, bool PINFO>
__global__ void __launch_bounds__(kEvThreads, 2) envelope_covariance_kernel(const WindowArgs a, double* ws, size_t ws_stride, int blocks_cap, double* cov, int32_t* mask, int32_t* status, const CovPairs pp) {
    constexpr int D = 6, DD = 36, RS = 13, S = kEvSlots;
    const int tid = threadIdx.x;
    const long long inst = blockIdx.x;
    const WindowCaps& cp = a.caps;
    const int nvm = cp.nv_max;
    const EnvLayout lay = env_layout(nvm);
    double* sinv = evlds + lay.sinv;
    double* rec = evlds + lay.rec;
    int* ib = reinterpret_cast<int*>(evlds + lay.ints);
    int* ei = ib + lay.ei;
    int* wc = ib + lay.wc;
    int* first = ib + lay.first;
    int* off = ib + lay.off;
    int* last = ib + lay.last;
    int* list = ib + lay.list;
    int* mk = ib + lay.mk;
    const int nv = a.counts[inst * 4 + 0], nr = a.counts[inst * 4 + 1], np = a.counts[inst * 4 + 2], ns = a.counts[inst * 4 + 3];
    const double* P = a.poses + (size_t)inst * nvm * 12;
    double* Hw = ws + (size_t)inst * ws_stride;       // [blocks_cap][36]  H -> the factor (S_j^-1, K_kj) -> Sigma
    double* Wc = Hw + (size_t)blocks_cap * DD;        // [nv_max][36]      the current column: H_kj (forward), Sigma_kj (backward), by list position
    double* dg = Wc + (size_t)nvm * DD;               // [nv_max][6]       diag(H) of every coordinate (the scale of the relative pivot test)
    const int slot = tid / DD, en = tid % DD, r = en / D, c = en % D;
    const bool ent = slot < S;
    // block (i, j), j <= i, of the envelope
    auto blk = [&](int i, int j) { return Hw + ((size_t)off[i] + (size_t)(j - first[i])) * DD; };

    // ---- profile ----------------------------------------------------------------------------------------------------------------------
    for (int v = tid; v < nv; v += kEvThreads) { first[v] = v; last[v] = v; }
    __syncthreads();
    for (int e = tid; e < nr; e += kEvThreads) {
        const int32_t* ix = a.r_idx + ((size_t)inst * cp.nr_max + e) * 2;
        if (ix[1] >= 0) atomicMin(&first[max(ix[0], ix[1])], min(ix[0], ix[1]));
    }
    for (int e = tid; e < ns; e += kEvThreads) {
        const int32_t* ix = a.s_idx + ((size_t)inst * cp.ns_max + e) * 4;
        atomicMin(&first[max(ix[0], ix[1])], min(ix[0], ix[1]));
    }
    if (JOINT) {   // a requested pair is one more edge (a structural zero): the selected inversion then leaves Sigma_ij in its block
        const int npr = min(pp.counts[inst], pp.npair_max);
        for (int p = tid; p < npr; p += kEvThreads) {
            const int32_t* ix = pp.pairs + ((size_t)inst * pp.npair_max + p) * 2;
            if (ix[0] >= 0 && ix[0] < nv && ix[1] >= 0 && ix[1] < nv) atomicMin(&first[max(ix[0], ix[1])], min(ix[0], ix[1]));
        }
    }
    __syncthreads();
    for (int v = tid; v < nv; v += kEvThreads) atomicMax(&last[first[v]], v);
    __syncthreads();
    if (tid == 0) {
        int at = 0, top = 0;
        for (int v = 0; v < nv; ++v) {
            off[v] = at;
            at += v - first[v] + 1;
            top = max(top, last[v]);
            last[v] = top;
        }
        off[nv] = at;
    }
    __syncthreads();
    const int total = off[nv];
    // (the host sized the workspace from these very tables: a larger envelope cannot be, and is refused rather than written)
    const bool fits = total <= blocks_cap;
    bool ok = fits;
    if (fits) {
        for (size_t k = tid; k < (size_t)total * DD; k += kEvThreads) Hw[k] = 0.0;

        // ---- linearisation + assembly ----------------------------------------------------------------------------------------------
        for (int e0 = 0; e0 < nr; e0 += kEvRangeChunk) {
            __syncthreads();
            const int e = e0 + tid;
            if (e < nr) {
                const int32_t* ix = a.r_idx + ((size_t)inst * cp.nr_max + e) * 2;
                cov_range_edge<D, JAC>(P, a.anchors, ix[0], ix[1], a.r_val + ((size_t)inst * cp.nr_max + e) * 5, rec + tid * RS);
                ei[2 * tid] = ix[0]; ei[2 * tid + 1] = ix[1];
            }
            __syncthreads();
            if (ent) {
                const int m = min(kEvRangeChunk, nr - e0);
                for (int k = 0; k < m; ++k) {
                    const double* q = rec + k * RS;
                    const int a0 = ei[2 * k], a1 = ei[2 * k + 1];
                    const double w = q[0];
                    if (a0 % S == slot) blk(a0, a0)[en] += w * (q[1 + r] * q[1 + c]);
                    if (a1 >= 0) {
                        if (a1 % S == slot) blk(a1, a1)[en] += w * (q[1 + D + r] * q[1 + D + c]);
                        if (a1 > a0) { if (a1 % S == slot) blk(a1, a0)[en] += w * (q[1 + D + r] * q[1 + c]); }   // rows: the later pose
                        else if (a0 % S == slot) blk(a0, a1)[en] += w * (q[1 + r] * q[1 + D + c]);
                    }
                }
            }
        }
        for (int e0 = 0; e0 < np; e0 += kEvPriorChunk) {
            __syncthreads();
            const int e = e0 + tid;
            if (tid < kEvPriorChunk && e < np) {
                const int v = a.p_idx[(size_t)inst * cp.np_max + e];
                if (PINFO) cov_prior_block_full(a.p_val + ((size_t)inst * cp.np_max + e) * 18, a.p_info + ((size_t)inst * cp.np_max + e) * 36, P + v * 12, rec + tid * 21);
                else cov_prior_block(a.p_val + ((size_t)inst * cp.np_max + e) * 18, P + v * 12, rec + tid * 21);
                ei[tid] = v;
            }
            __syncthreads();
            if (ent) {
                const int m = min(kEvPriorChunk, np - e0);
                for (int k = 0; k < m; ++k) {
                    const int v = ei[k];
                    if (v % S == slot) blk(v, v)[en] += rec[k * 21 + LOCAMD_CV_TRI(r, c)];
                }
            }
        }
        for (int e0 = 0; e0 < ns; e0 += kEvSe3Chunk) {
            __syncthreads();
            const int e = e0 + tid;
            if (tid < kEvSe3Chunk && e < ns) {
                const int32_t* ix = a.s_idx + ((size_t)inst * cp.ns_max + e) * 4;
                const int vi = ix[0], vj = ix[1];
                double Xi[12], Xj[12], bi[6], bj[6], rterm;
#pragma unroll
                for (int k = 0; k < 12; ++k) { Xi[k] = P[vi * 12 + k]; Xj[k] = P[vj * 12 + k]; }
                double* q = rec + tid * kCovSRec;
                chain_se3_terms<true>(Xi, Xj, a.s_val + ((size_t)inst * cp.ns_max + e) * 48, ix[2] != 0, vj > vi, q, q + 21, q + 42, bi, bj, rterm);
                ei[2 * tid] = vi; ei[2 * tid + 1] = vj;
            }
            __syncthreads();
            if (ent) {
                const int m = min(kEvSe3Chunk, ns - e0);
                for (int k = 0; k < m; ++k) {
                    const double* q = rec + k * kCovSRec;
                    const int vi = ei[2 * k], vj = ei[2 * k + 1];
                    if (vi % S == slot) blk(vi, vi)[en] += q[LOCAMD_CV_TRI(r, c)];
                    if (vj % S == slot) blk(vj, vj)[en] += q[21 + LOCAMD_CV_TRI(r, c)];
                    const int hi = max(vi, vj);
                    if (hi % S == slot) blk(hi, min(vi, vj))[en] += q[42 + 6 * c + r];   // rows: the later pose
                }
            }
        }
        __syncthreads();
        // ---- excluded coordinates: a diagonal entry exactly 0 (its row and column are 0 as well) -----------------------------------------
        for (int v = tid; v < nv; v += kEvThreads) mk[v] = cov_exclude_zero_diagonal<D>(blk(v, v), dg + (size_t)v * D);
        __syncthreads();

        // ---- forward: column after column -----------------------------------------------------------------------------------------------
        for (int j = 0; j < nv; ++j) {
            const int m = env_column_rows(j, first, last, list, wc, tid);
            double* Sj = blk(j, j);
            double Li[D][D];
            cov_chol_inverse<D>(Sj, dg + (size_t)j * D, ok, Li);   // (every thread: the verdict needs no exchange)
            double si = 0.0;   // entry (r, c) of S_j^-1 = L^-T L^-1 (static indices: Li stays in registers)
#pragma unroll
            for (int r2 = 0; r2 < D; ++r2)
#pragma unroll
                for (int c2 = 0; c2 < D; ++c2) {
                    double s = 0.0;
#pragma unroll
                    for (int k = (r2 > c2 ? r2 : c2); k < D; ++k) s = __builtin_fma(Li[k][r2], Li[k][c2], s);
                    si = (r2 == r && c2 == c) ? s : si;
                }
            __syncthreads();   // (S_j is read)
            if (slot == 0) { sinv[en] = si; Sj[en] = si; }
            if (m > 0 && m <= kEvLdsRows) {
                // the column in LDS (the record region is free after the assembly): H_kj in Wl, K_kj in Kl — the update reads nothing else
                double* Wl = rec;
                double* Kl = rec + m * DD;
                if (ent)
                    for (int q = slot; q < m; q += S) Wl[q * DD + en] = blk(list[q], j)[en];
                __syncthreads();
                if (ent)
                    for (int q = slot; q < m; q += S) {   // K_kj = H_kj S_j^-1
                        const double* h = Wl + q * DD + r * D;
                        double kr = 0.0;
#pragma unroll
                        for (int t = 0; t < D; ++t) kr = __builtin_fma(h[t], sinv[t * D + c], kr);
                        Kl[q * DD + en] = kr;
                        blk(list[q], j)[en] = kr;
                    }
                __syncthreads();
                if (ent) {   // H_ik -= K_ij H_jk over the pairs (a, b), b <= a, of the list
                    const int pairs = m * (m + 1) / 2;
                    int pa = 0, pb = slot;
                    while (pb > pa) { pb -= pa + 1; ++pa; }
                    for (int p = slot; p < pairs; p += S) {
                        const double* kk = Kl + pa * DD + r * D;
                        const double* h = Wl + pb * DD + c * D;
                        double s = 0.0;
#pragma unroll
                        for (int t = 0; t < D; ++t) s = __builtin_fma(kk[t], h[t], s);
                        blk(list[pa], list[pb])[en] -= s;
                        pb += S;
                        while (pb > pa) { pb -= pa + 1; ++pa; }
                    }
                }
            } else if (m > 0) {   // a column too tall for the LDS: the same steps through the workspace's column array
                if (ent)
                    for (int q = slot; q < m; q += S) Wc[(size_t)q * DD + en] = blk(list[q], j)[en];
                __syncthreads();
                if (ent)
                    for (int q = slot; q < m; q += S) {   // K_kj = H_kj S_j^-1
                        const double* h = Wc + (size_t)q * DD + r * D;
                        double kr = 0.0;
#pragma unroll
                        for (int t = 0; t < D; ++t) kr = __builtin_fma(h[t], sinv[t * D + c], kr);
                        blk(list[q], j)[en] = kr;
                    }
                __syncthreads();
                if (ent) {   // H_ik -= K_ij H_jk over the pairs (a, b), b <= a, of the list
                    const long long pairs = (long long)m * (m + 1) / 2;
                    int pa = 0, pb = slot;
                    while (pb > pa) { pb -= pa + 1; ++pa; }
                    for (long long p = slot; p < pairs; p += S) {
                        const int ka = list[pa], kb = list[pb];
                        const double* kk = blk(ka, j) + r * D;
                        const double* h = Wc + (size_t)pb * DD + c * D;
                        double s = 0.0;
#pragma unroll
                        for (int t = 0; t < D; ++t) s = __builtin_fma(kk[t], h[t], s);
                        blk(ka, kb)[en] -= s;
                        pb += S;
                        while (pb > pa) { pb -= pa + 1; ++pa; }
                    }
                }
            }
            __syncthreads();
        }

        // ---- backward: the selected inverse on the same structure ---------------------------------------------------------------------------
        for (int j = nv - 1; j >= 0; --j) {
            const int m = env_column_rows(j, first, last, list, wc, tid);
            if (m > 0 && m <= kEvLdsRows) {
                // the column in LDS: K_kj in Kl, then Sigma_kj in Wl; nothing reads column j from the workspace after the first step,
                // so Sigma_kj goes to its place at once
                double* Wl = rec;
                double* Kl = rec + m * DD;
                if (ent)
                    for (int q = slot; q < m; q += S) Kl[q * DD + en] = blk(list[q], j)[en];
                __syncthreads();
                if (ent)
                    for (int q = slot; q < m; q += S) {   // Sigma_ij = -sum_k Sigma_ik K_kj
                        const int i = list[q];
                        double s = 0.0;
                        for (int p = 0; p < m; ++p) {
                            const int k = list[p];
                            const double* kk = Kl + p * DD;
                            if (i >= k) {
                                const double* sg = blk(i, k) + r * D;
#pragma unroll
                                for (int t = 0; t < D; ++t) s = __builtin_fma(sg[t], kk[t * D + c], s);
                            } else {
                                const double* sg = blk(k, i) + r;
#pragma unroll
                                for (int t = 0; t < D; ++t) s = __builtin_fma(sg[t * D], kk[t * D + c], s);
                            }
                        }
                        Wl[q * DD + en] = -s;
                        blk(i, j)[en] = -s;
                    }
                __syncthreads();
                if (slot == 0) {   // Sigma_jj = S_j^-1 - sum_k K_kj^T Sigma_kj
                    double sj = blk(j, j)[en];
                    for (int p = 0; p < m; ++p) {
                        const double* kk = Kl + p * DD;
                        const double* sg = Wl + p * DD;
#pragma unroll
                        for (int t = 0; t < D; ++t) sj = __builtin_fma(-kk[t * D + r], sg[t * D + c], sj);
                    }
                    blk(j, j)[en] = sj;
                }
            } else if (m > 0) {
                if (ent)
                    for (int q = slot; q < m; q += S) {   // Sigma_ij = -sum_k Sigma_ik K_kj
                        const int i = list[q];
                        double s = 0.0;
                        for (int p = 0; p < m; ++p) {
                            const int k = list[p];
                            const double* kk = blk(k, j);
                            if (i >= k) {
                                const double* sg = blk(i, k) + r * D;
#pragma unroll
                                for (int t = 0; t < D; ++t) s = __builtin_fma(sg[t], kk[t * D + c], s);
                            } else {
                                const double* sg = blk(k, i) + r;
#pragma unroll
                                for (int t = 0; t < D; ++t) s = __builtin_fma(sg[t * D], kk[t * D + c], s);
                            }
                        }
                        Wc[(size_t)q * DD + en] = -s;
                    }
                __syncthreads();
                double sj = 0.0;
                if (slot == 0) {   // Sigma_jj = S_j^-1 - sum_k K_kj^T Sigma_kj
                    sj = blk(j, j)[en];
                    for (int p = 0; p < m; ++p) {
                        const double* kk = blk(list[p], j);
                        const double* sg = Wc + (size_t)p * DD;
#pragma unroll
                        for (int t = 0; t < D; ++t) sj = __builtin_fma(-kk[t * D + r], sg[t * D + c], sj);
                    }
                }
                __syncthreads();   // (K_kj is read)
                if (slot == 0) blk(j, j)[en] = sj;
                if (ent)
                    for (int q = slot; q < m; q += S) blk(list[q], j)[en] = Wc[(size_t)q * DD + en];
            }
            __syncthreads();
        }
    }

    // ---- output (cov_store_window's rules): blocks symmetrised, excluded rows / columns 0, slots >= nv 0, NaN for a singular window ---------
    double* out = cov + (size_t)inst * nvm * 36;
    for (int k = tid; k < nvm * 36; k += kEvThreads) {
        const int v = k / 36, rr = (k % 36) / 6, cc = k % 6;
        double x = 0.0;
        if (v < nv) {
            if (!ok) x = __builtin_nan("");
            else if (!((mk[v] >> rr) & 1) && !((mk[v] >> cc) & 1)) {
                const double* sg = blk(v, v);
                x = (sg[rr * D + cc] + sg[cc * D + rr]) * 0.5;
            }
        }
        out[k] = x;
    }
    for (int v = tid; v < nvm; v += kEvThreads) mask[(size_t)inst * nvm + v] = (v < nv && fits) ? mk[v] : 0;
    if (tid == 0) status[inst] = ok ? 0 : -6;   // LOC_OK / LOC_ERR_SINGULAR

    // ---- joint calls: Sigma_ij from the block (max, min) of the envelope, thread = (pair, entry); (i, i) as the store above ----------------------
    if (JOINT) {
        const int npr = pp.counts[inst];
        const int32_t* pr = pp.pairs + (size_t)inst * pp.npair_max * 2;
        double* xo = pp.cross + (size_t)inst * pp.npair_max * 36;
        for (int k = tid; k < pp.npair_max * 36; k += kEvThreads) {
            const int p = k / 36, rr = (k % 36) / 6, cc = k % 6;
            const int pi = p < npr ? pr[2 * p] : -1, pj = p < npr ? pr[2 * p + 1] : -1;
            double x = 0.0;
            if (pi >= 0 && pi < nv && pj >= 0 && pj < nv) {
                if (!ok) x = __builtin_nan("");
                else if (!((mk[pi] >> rr) & 1) && !((mk[pj] >> cc) & 1)) {
                    if (pi == pj) { const double* sg = blk(pi, pi); x = (sg[rr * D + cc] + sg[cc * D + rr]) * 0.5; }
                    else x = pi > pj ? blk(pi, pj)[rr * D + cc] : blk(pj, pi)[cc * D + rr];   // (rows of a stored block: the later pose)
                }
            }
            xo[k] = x;
        }
    }
}

template <int JAC, bool JOINT, bool PINFO>
hipError_t launch_env_cov_p(const WindowArgs& a, double* ws, size_t ws_stride, int blocks, size_t lds, double* cov, int32_t* mask, int32_t* status, const CovPairs& pp, hipStream_t stream) {
    const hipError_t e = allow_dynamic_lds<&envelope_covariance_kernel<JAC, JOINT, PINFO>>((int)kCovMaxLds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((envelope_covariance_kernel<JAC, JOINT, PINFO>), dim3((unsigned)a.B), dim3(kEvThreads), lds, stream, a, ws, ws_stride, blocks, cov, mask, status, pp);
    return hipGetLastError();
}
template <int JAC, bool JOINT>
hipError_t launch_env_cov_j(const WindowArgs& a, double* ws, size_t ws_stride, int blocks, size_t lds, double* cov, int32_t* mask, int32_t* status, const CovPairs& pp, hipStream_t stream) {
    return a.p_info ? launch_env_cov_p<JAC, JOINT, true>(a, ws, ws_stride, blocks, lds, cov, mask, status, pp, stream)
                    : launch_env_cov_p<JAC, JOINT, false>(a, ws, ws_stride, blocks, lds, cov, mask, status, pp, stream);
}
template <int JAC>
hipError_t launch_env_cov_t(const WindowArgs& a, double* ws, size_t ws_stride, int blocks, size_t lds, double* cov, int32_t* mask, int32_t* status, const CovPairs& pp, hipStream_t stream) {
    return pp.cross ? launch_env_cov_j<JAC, true>(a, ws, ws_stride, blocks, lds, cov, mask, status, pp, stream)
                    : launch_env_cov_j<JAC, false>(a, ws, ws_stride, blocks, lds, cov, mask, status, pp, stream);
}

}  // namespace

size_t window_envelope_covariance_lds_bytes(const WindowCaps& c) { return env_layout(c.nv_max).bytes; }

size_t window_envelope_covariance_workspace_doubles(const WindowCaps& c, long long blocks) {
    return ((size_t)blocks + (size_t)c.nv_max) * 36 + (size_t)c.nv_max * 6;
}

hipError_t launch_window_envelope_covariance(const WindowArgs& a, double* ws, long long blocks, double* cov, int32_t* mask, int32_t* status, const CovPairs& pp, hipStream_t stream) {
    if (a.B <= 0) return hipSuccess;
    if (!ws || blocks < 0 || blocks > (1ll << 30)) return hipErrorInvalidValue;
    if (!cov_envelope_fits(a.caps)) return hipErrorInvalidValue;
    const size_t lds = env_layout(a.caps.nv_max).bytes;
    const size_t stride = window_envelope_covariance_workspace_doubles(a.caps, blocks);
    return a.jacobian ? launch_env_cov_t<1>(a, ws, stride, (int)blocks, lds, cov, mask, status, pp, stream)
                      : launch_env_cov_t<0>(a, ws, stride, (int)blocks, lds, cov, mask, status, pp, stream);
}

}  // namespace locamd
