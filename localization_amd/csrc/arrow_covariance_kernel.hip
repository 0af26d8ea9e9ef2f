// gfx950 (MI355X / CDNA4): marginal covariances of translation-only ARROWHEAD windows (BASELINE config 4, anchor self-calibration: a tag
// trajectory whose poses range to up to 12 nodes that are unknowns themselves — the windows arrow3_lm_kernel solves), one workgroup
// of four waves per window.
//
// What it computes: DESIGN.md §2 word for word — covariance_kernel.hip's definition with 3 x 3 blocks (the rotation bits always set).
// The split is the kernel's own and trivial: border = the window's last nb pose slots, nb = the smallest number such that every
// pose-to-pose edge between non-consecutive slots has an endpoint there (capi_window.cpp: build_arrow_aux's rule, recomputed here from
// r_idx); chain = the nc = nv - nb slots before it, one segment, no separators.  With
//   H = [ A  B ; B^T  C ],   A block-tridiagonal (nc blocks), B dense 3 nc x 3 nb, C dense 3 nb x 3 nb (3 nb <= 36),
//   Y = A^-1 B,   S = C - B^T Y:   [H^-1]_border = S^-1,   [H^-1]_ii = [A^-1]_ii + Y_i S^-1 Y_i^T  (chain pose i).
// The pivot test (cov_block_device.h: cov_pivot_above_noise, kCovRelPivot of the coordinate's diagonal entry of H) covers A's block pivots
// (step 3) and S's Cholesky pivots (step 5).
//
// Schedule (no atomics; every sum is taken in edge order by the one thread that owns its entry: the same bits on every run):
//   1. linearise, lane = edge, chunks of 256: the record (rho' info, J0, J1) goes to LDS and to the window's HBM workspace.  Of every
//      chunk the border threads (lane = entry (r, c) of border slot b) add their shares of C from LDS, and the pose threads
//      (lane = chain pose) note which edges touch their pose (a list per pose in the workspace, `cap` entries each);
//   2. assemble, lane = chain pose: the pose's list gives H_ii, H_{i+1,i} (LDS) and the pose's rows of B (workspace, [chain row][36]);
//   3. factor A, one lane: S_0 = H_00, K_i = H_{i+1,i} S_i^-1, S_{i+1} = H_{i+1,i+1} - K_i H_{i,i+1} (covariance_kernel.hip's recurrence).  The
//      3 x 3 Cholesky and L^-1 are cov_chol_inverse's loops written out: called through that function (and with cov_range_edge for the
//      fetch of step 1) the pass measured 1 % slower than before, more than its run-to-run spread;
//   4. solve A Y = B, lane = border column: forward w_i = S_i^-1 (b_i - K_{i-1} z_{i-1}), backward y_i = w_i - K_i^T y_{i+1}; the backward
//      sweep also sums the lane's column of B^T Y in registers.  A lane of another wave meanwhile runs the chain pass's selected
//      inversion Sigma_i = S_i^-1 + K_i^T Sigma_{i+1} K_i for [A^-1]_ii;
//   5. S = C - B^T Y, its Cholesky factor and inverse in LDS (lane = row / column);
//   6. chain marginals, lane = chain pose; 7. the store (cov_store_window's rules); 8. joint calls only: the cross blocks, lane = pair.
#include "cov_block_device.h"
#include "window_kernel.h"

namespace locamd {

namespace {

extern __shared__ double aclds[];

template <int JAC, bool JOINT>
__global__ void __launch_bounds__(kAcThreads) arrow_covariance_kernel(const WindowArgs a, double* ws, int cap, double* cov, int32_t* mask, int32_t* status, const CovPairs pp) {
    constexpr int BS = kAcBS;
    const int tid = threadIdx.x;
    const long long inst = blockIdx.x;
    const WindowCaps& cp = a.caps;
    const int nvm = cp.nv_max;
    const ArrowCovLayout lay = arrow_cov_layout(nvm);
    double* Hd = aclds + lay.hd;
    double* Ho = aclds + lay.ho;
    double* dg = aclds + lay.dg;
    double* C = aclds + lay.cc;
    double* ig = aclds + lay.ig;
    double* rec = aclds + lay.rec;
    double* Li = rec;
    int* ib = reinterpret_cast<int*>(aclds + lay.ints);
    int* ei = ib + lay.ei;
    int* cnt = ib + lay.cnt;
    int* mk = ib + lay.mk;
    int* flag = ib + lay.flag;
    const int nv = a.counts[inst * 4 + 0], nr = a.counts[inst * 4 + 1], np = a.counts[inst * 4 + 2];
    const double* P = a.poses + (size_t)inst * nvm * 12;
    const int32_t* RI = a.r_idx + (size_t)inst * cp.nr_max * 2;
    const double* RV = a.r_val + (size_t)inst * cp.nr_max * 5;
    const int32_t* PI = a.p_idx + (size_t)inst * cp.np_max;
    const double* PV = a.p_val + (size_t)inst * cp.np_max * 18;
    double* wsw = ws + (size_t)inst * arrow_cov_ws_doubles(cp, cap);
    double* grec = wsw;                                   // [nr_max][8]
    double* Bm = grec + (size_t)cp.nr_max * kAcRecG;      // [3 nv_max][36]
    double* Ym = Bm + (size_t)nvm * 3 * BS;               // [3 nv_max][36]
    int32_t* lst = reinterpret_cast<int32_t*>(Ym + (size_t)nvm * 3 * BS);   // [nv_max][cap]: edge e, or -1 - prior

    // ---- the border: the last nb slots ------------------------------------------------------------------------------------------------
    if (tid == 0) { flag[0] = 0; flag[1] = 1; }
    for (int k = tid; k < BS * BS; k += kAcThreads) C[k] = 0.0;
    for (int k = tid; k < nvm; k += kAcThreads) { cnt[k] = 0; mk[k] = 0; }
    __syncthreads();
    {
        int m = 0;
        for (int e = tid; e < nr; e += kAcThreads) {
            const int v0 = RI[2 * e], v1 = RI[2 * e + 1];
            if (v1 < 0) continue;
            const int hi = max(v0, v1), lo = min(v0, v1);
            if (hi - lo != 1) m = max(m, nv - hi);
        }
        if (m > 0) atomicMax(&flag[0], m);   // (an integer maximum in LDS: the same value in any order)
    }
    __syncthreads();
    // (the host admits windows with 1 <= nb <= 12 and nc >= 2 only; anything else here is reported as singular, never indexed with)
    const int nb = flag[0];
    const bool shape_ok = nb >= 1 && nb <= 12 && nv - nb >= 2 && nv <= nvm;
    const int nc = shape_ok ? nv - nb : 0;
    const int D = shape_ok ? 3 * nb : 0;
    for (int k = tid; k < nc * 3 * BS; k += kAcThreads) Bm[k] = 0.0;

    // ---- 1. linearisation; C; the poses' edge lists ----------------------------------------------------------------------------------------
    const int bb = tid / 9, br = (tid % 9) / 3, bc = tid % 3;   // border thread: entry (br, bc) of the blocks of border slot bb
    const bool bth = tid < 9 * nb && shape_ok;
    for (int e0 = 0; e0 < nr && shape_ok; e0 += kAcChunk) {
        __syncthreads();
        const int e = e0 + tid;
        if (e < nr) {
            const double* val = RV + (size_t)e * 5;
            const int v0 = RI[2 * e], v1 = RI[2 * e + 1];
            double X0[12], X1[12], p1[3];
#pragma unroll
            for (int k = 0; k < 12; ++k) X0[k] = P[v0 * 12 + k];
            const int v1c = v1 >= 0 ? v1 : v0;
#pragma unroll
            for (int k = 0; k < 12; ++k) X1[k] = P[v1c * 12 + k];
            if (v1 >= 0) { p1[0] = X1[9]; p1[1] = X1[10]; p1[2] = X1[11]; }
            else { const double* an = a.anchors + (size_t)(-1 - v1) * 3; p1[0] = an[0]; p1[1] = an[1]; p1[2] = an[2]; }
            double q[kAcRec];
            cov_range_rec<3, JAC>(X0, X1, p1, v1 >= 0, val, q);
#pragma unroll
            for (int k = 0; k < kAcRec; ++k) { rec[tid * kAcRec + k] = q[k]; grec[(size_t)e * kAcRecG + k] = q[k]; }
            ei[2 * tid] = v0; ei[2 * tid + 1] = v1;
        }
        __syncthreads();
        const int m = min(kAcChunk, nr - e0);
        for (int v = tid; v < nc; v += kAcThreads) {
            int n = cnt[v];
            for (int k = 0; k < m; ++k)
                if (ei[2 * k] == v || ei[2 * k + 1] == v) { if (n < cap) lst[(size_t)v * cap + n] = e0 + k; ++n; }
            cnt[v] = n;
        }
        if (bth) {
            const int vb = nc + bb;
            for (int k = 0; k < m; ++k) {
                const int a0 = ei[2 * k], a1 = ei[2 * k + 1];
                if (a0 != vb && a1 != vb) continue;
                const double* q = rec + k * kAcRec;
                const double* Jm = a0 == vb ? q + 1 : q + 4;   // the border slot's own columns
                const double* Jo = a0 == vb ? q + 4 : q + 1;
                const int vo = a0 == vb ? a1 : a0;
                C[(3 * bb + br) * BS + 3 * bb + bc] += q[0] * (Jm[br] * Jm[bc]);
                if (vo >= nc && vo != vb) C[(3 * bb + br) * BS + 3 * (vo - nc) + bc] += q[0] * (Jm[br] * Jo[bc]);
            }
        }
    }
    for (int e0 = 0; e0 < np && shape_ok; e0 += kAcChunk) {
        __syncthreads();
        const int e = e0 + tid;
        if (e < np) {
            const int v = PI[e];
            double q[21];
            cov_prior_block(PV + (size_t)e * 18, P + v * 12, q);
#pragma unroll
            for (int k = 0; k < 6; ++k) rec[tid * kAcRec + k] = q[k];   // the translation block (lower triangle)
            ei[tid] = v;
        }
        __syncthreads();
        const int m = min(kAcChunk, np - e0);
        for (int v = tid; v < nc; v += kAcThreads) {
            int n = cnt[v];
            for (int k = 0; k < m; ++k)
                if (ei[k] == v) { if (n < cap) lst[(size_t)v * cap + n] = -1 - (e0 + k); ++n; }
            cnt[v] = n;
        }
        if (bth) {
            const int vb = nc + bb;
            for (int k = 0; k < m; ++k)
                if (ei[k] == vb) C[(3 * bb + br) * BS + 3 * bb + bc] += rec[k * kAcRec + LOCAMD_CV_TRI(br, bc)];
        }
    }
    __syncthreads();   // (the records in the workspace and the lists were written by other threads of this workgroup)

    // ---- 2. assembly of A and B, lane = chain pose ---------------------------------------------------------------------------------------
    for (int v = tid; v < nc; v += kAcThreads) {
        double h[6] = {0, 0, 0, 0, 0, 0};           // H_vv, lower triangle
        double o[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};  // H_{v+1,v}
        const int n = cnt[v];
        if (n > cap) flag[1] = 0;   // (cannot happen: `cap` is the batch's largest list, counted by the host)
        double* Bv = Bm + (size_t)v * 3 * BS;
        for (int k = 0; k < min(n, cap); ++k) {
            const int e = lst[(size_t)v * cap + k];
            if (e >= 0) {
                const double* q = grec + (size_t)e * kAcRecG;
                const int a0 = RI[2 * e], a1 = RI[2 * e + 1];
                const bool first = a0 == v;
                const int vo = first ? a1 : a0;
                double Jm[3], Jo[3];
                const double w = q[0];
#pragma unroll
                for (int j = 0; j < 3; ++j) { Jm[j] = first ? q[1 + j] : q[4 + j]; Jo[j] = first ? q[4 + j] : q[1 + j]; }
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c <= r; ++c) h[r * (r + 1) / 2 + c] += w * (Jm[r] * Jm[c]);
                if (vo == v + 1 && vo < nc) {
#pragma unroll
                    for (int r = 0; r < 3; ++r)
#pragma unroll
                        for (int c = 0; c < 3; ++c) o[r * 3 + c] += w * (Jo[r] * Jm[c]);   // rows: the later pose
                } else if (vo >= nc) {
                    const int b = vo - nc;
#pragma unroll
                    for (int r = 0; r < 3; ++r)
#pragma unroll
                        for (int c = 0; c < 3; ++c) Bv[r * BS + 3 * b + c] += w * (Jm[r] * Jo[c]);
                }
            } else {
                const int pe = -1 - e;
                double q[21];
                cov_prior_block(PV + (size_t)pe * 18, P + v * 12, q);
#pragma unroll
                for (int j = 0; j < 6; ++j) h[j] += q[j];
            }
        }
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) Hd[v * 9 + r * 3 + c] = h[LOCAMD_CV_TRI(r, c)];
#pragma unroll
        for (int j = 0; j < 9; ++j) Ho[v * 9 + j] = o[j];
        // excluded coordinates: a diagonal entry exactly 0 (its row and column are 0 as well)
        mk[v] = cov_exclude_zero_diagonal<3>(Hd + v * 9, dg + v * 3);
    }
    if (tid < nb) {
        int bits = 0x38;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            double& d = C[(3 * tid + k) * BS + 3 * tid + k];
            if (d == 0.0) { bits |= 1 << k; d = 1.0; }
            dg[(nc + tid) * 3 + k] = d;
        }
        mk[nc + tid] = bits;
    }
    __syncthreads();

    // ---- 3. block-tridiagonal factorisation of A, one lane: Hd[i] = S_i^-1, Ho[i] = K_i ----------------------------------------------------
    if (tid == 0 && nc > 0) {
        bool ok = true;
        double S[3][3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) S[r][c] = Hd[r * 3 + c];
        for (int i = 0; i < nc; ++i) {
            double A[3][3];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) A[r][c] = S[r][c];
            double g[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                ok = ok && cov_pivot_above_noise(A[j][j], dg[i * 3 + j]);
                g[j] = pivot_rsqrt(A[j][j]);
#pragma unroll
                for (int i2 = j + 1; i2 < 3; ++i2) A[i2][j] *= g[j];
#pragma unroll
                for (int i2 = j + 1; i2 < 3; ++i2)
#pragma unroll
                    for (int c = j + 1; c <= i2; ++c) A[i2][c] = __builtin_fma(-A[i2][j], A[c][j], A[i2][c]);
            }
            ok = ok && (g[0] + g[1] + g[2]) < DBL_MAX;   // (a pivot <= 0 or not finite: NaN / inf — window_kernel.hip's test)
            double L[3][3];   // L^-1 (lower)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                L[c][c] = g[c];
#pragma unroll
                for (int r = c + 1; r < 3; ++r) {
                    double s = 0.0;
#pragma unroll
                    for (int k = c; k < r; ++k) s = __builtin_fma(A[r][k], L[k][c], s);
                    L[r][c] = -g[r] * s;
                }
            }
            double Si[3][3];   // S_i^-1 = L^-T L^-1
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c <= r; ++c) {
                    double s = 0.0;
#pragma unroll
                    for (int k = r; k < 3; ++k) s = __builtin_fma(L[k][r], L[k][c], s);
                    Si[r][c] = s; Si[c][r] = s;
                }
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) Hd[i * 9 + r * 3 + c] = Si[r][c];
            if (i + 1 < nc) {
                double O[3][3], K[3][3];
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c) O[r][c] = Ho[i * 9 + r * 3 + c];
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        double s = 0.0;
#pragma unroll
                        for (int k = 0; k < 3; ++k) s = __builtin_fma(O[r][k], Si[k][c], s);
                        K[r][c] = s;
                    }
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        double s = 0.0;   // (K_i H_{i,i+1})_rc
#pragma unroll
                        for (int k = 0; k < 3; ++k) s = __builtin_fma(K[r][k], O[c][k], s);
                        S[r][c] = Hd[(i + 1) * 9 + r * 3 + c] - s;
                        Ho[i * 9 + r * 3 + c] = K[r][c];
                    }
            }
        }
        if (!ok) flag[1] = 0;
    }
    __syncthreads();

    // ---- 4. A Y = B, lane = border column ------------------------------------------------------------------------------------------------------
    const int q = tid;
    if (q < D) {   // forward: w_i = S_i^-1 (b_i - K_{i-1} z_{i-1})
        double z[3] = {0, 0, 0};
        for (int i = 0; i < nc; ++i) {
            double b[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) b[r] = Bm[(size_t)(3 * i + r) * BS + q];
            if (i > 0) {
                const double* K = Ho + (i - 1) * 9;
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int k = 0; k < 3; ++k) b[r] = __builtin_fma(-K[r * 3 + k], z[k], b[r]);
            }
            const double* Si = Hd + i * 9;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                z[r] = b[r];
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < 3; ++k) s = __builtin_fma(Si[r * 3 + k], b[k], s);
                Ym[(size_t)(3 * i + r) * BS + q] = s;
            }
        }
    }
    __syncthreads();
    if (q < D) {   // backward: y_i = w_i - K_i^T y_{i+1}; the lane's column of B^T Y
        double acc[BS];
#pragma unroll
        for (int p = 0; p < BS; ++p) acc[p] = 0.0;
        double y[3] = {0, 0, 0};
        for (int i = nc - 1; i >= 0; --i) {
            double w[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) w[r] = Ym[(size_t)(3 * i + r) * BS + q];
            if (i + 1 < nc) {
                const double* K = Ho + i * 9;
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int k = 0; k < 3; ++k) w[r] = __builtin_fma(-K[k * 3 + r], y[k], w[r]);
            }
#pragma unroll
            for (int r = 0; r < 3; ++r) { y[r] = w[r]; Ym[(size_t)(3 * i + r) * BS + q] = w[r]; }
            const double* Bi = Bm + (size_t)(3 * i) * BS;
#pragma unroll
            for (int p = 0; p < BS; ++p) {
                if (p < D) {
#pragma unroll
                    for (int r = 0; r < 3; ++r) acc[p] = __builtin_fma(Bi[r * BS + p], y[r], acc[p]);
                }
            }
        }
#pragma unroll
        for (int p = 0; p < BS; ++p)
            if (p < D) C[p * BS + q] -= acc[p];   // S = C - B^T Y
    } else if (tid == 64 && nc > 0) {
        // the chain pass's selected inversion, in place: [A^-1]_ii = S_i^-1 + K_i^T [A^-1]_{i+1,i+1} K_i
        double G[3][3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) G[r][c] = Hd[(nc - 1) * 9 + r * 3 + c];
        for (int i = nc - 2; i >= 0; --i) {
            double K[3][3], T[3][3];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) K[r][c] = Ho[i * 9 + r * 3 + c];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    double s = 0.0;
#pragma unroll
                    for (int k = 0; k < 3; ++k) s = __builtin_fma(G[r][k], K[k][c], s);
                    T[r][c] = s;
                }
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    double s = Hd[i * 9 + r * 3 + c];
#pragma unroll
                    for (int k = 0; k < 3; ++k) s = __builtin_fma(K[k][r], T[k][c], s);
                    G[r][c] = s;
                }
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) Hd[i * 9 + r * 3 + c] = G[r][c];
        }
    }
    __syncthreads();

    // ---- 5. S = L L^T (lane = row, column after column, pivots checked), L^-1 (lane = column), S^-1 = L^-T L^-1 ----------------------------
    for (int j = 0; j < D; ++j) {
        double s = 0.0;
        if (tid >= j && tid < D) {
            s = C[tid * BS + j];
            for (int k = 0; k < j; ++k) s = __builtin_fma(-C[tid * BS + k], C[j * BS + k], s);
        }
        if (tid == j) {
            const double g = pivot_rsqrt(s);
            if (!cov_pivot_above_noise(s, dg[nc * 3 + j]) || !(g < DBL_MAX)) flag[1] = 0;
            ig[j] = g;
            C[j * BS + j] = s * g;
        }
        __syncthreads();
        if (tid > j && tid < D) C[tid * BS + j] = s * ig[j];
        __syncthreads();
    }
    if (tid < D) {
        const int c = tid;
        for (int r = 0; r < D; ++r) {
            double x = 0.0;
            if (r >= c) {
                x = r == c ? 1.0 : 0.0;
                for (int k = c; k < r; ++k) x = __builtin_fma(-C[r * BS + k], Li[k * BS + c], x);
                x *= ig[r];
            }
            Li[r * BS + c] = x;
        }
    }
    __syncthreads();
    if (tid < D) {
        const int c = tid;
        for (int r = 0; r < D; ++r) {
            double s = 0.0;
            for (int k = max(r, c); k < D; ++k) s = __builtin_fma(Li[k * BS + r], Li[k * BS + c], s);
            C[r * BS + c] = s;
        }
    }
    __syncthreads();

    // ---- 6. chain marginals, lane = chain pose: Sigma_ii = [A^-1]_ii + Y_i S^-1 Y_i^T ---------------------------------------------------------
    for (int v = tid; v < nc; v += kAcThreads) {
        const double* Yv = Ym + (size_t)v * 3 * BS;
        for (int r = 0; r < 3; ++r) {
            double y[BS];
#pragma unroll
            for (int k = 0; k < BS; ++k) y[k] = k < D ? Yv[r * BS + k] : 0.0;
            double acc[3] = {0, 0, 0};
            for (int p = 0; p < D; ++p) {
                double zp = 0.0;   // (S^-1 y_r)_p
#pragma unroll
                for (int k = 0; k < BS; ++k) zp = __builtin_fma(C[p * BS + k], y[k], zp);
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[c] = __builtin_fma(Yv[c * BS + p], zp, acc[c]);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) Hd[v * 9 + c * 3 + r] += acc[c];
        }
    }
    __syncthreads();

    // ---- 7. output: symmetric 6x6 per slot, excluded rows / columns 0, slots >= nv 0, NaN for a singular window ------------------------------
    const bool ok = flag[1] != 0 && shape_ok;
    double* out = cov + (size_t)inst * nvm * 36;
    for (int k = tid; k < nvm * 36; k += kAcThreads) {
        const int v = k / 36, rr = (k % 36) / 6, cc = k % 6;
        double x = 0.0;
        if (v < nv) {
            if (!ok) x = __builtin_nan("");
            else if (rr < 3 && cc < 3 && !((mk[v] >> rr) & 1) && !((mk[v] >> cc) & 1)) {
                if (v < nc) x = (Hd[v * 9 + rr * 3 + cc] + Hd[v * 9 + cc * 3 + rr]) * 0.5;
                else { const int b = 3 * (v - nc); x = (C[(b + rr) * BS + b + cc] + C[(b + cc) * BS + b + rr]) * 0.5; }
            }
        }
        out[k] = x;
    }
    for (int v = tid; v < nvm; v += kAcThreads) mask[(size_t)inst * nvm + v] = v < nv ? (shape_ok ? mk[v] : 0x38) : 0;
    if (tid == 0) status[inst] = ok ? 0 : -6;   // LOC_OK / LOC_ERR_SINGULAR

    // ---- 8. joint calls, lane = pair: the block (lo, hi) of H^-1 from S^-1 (C), Y (workspace), K_i (Ho) and Sigma_ii (Hd), transposed for (hi, lo) ----
    //   border - border: the block of S^-1;   chain i - border: -Y_i S^-1;
    //   chain - chain:   [A^-1]_ij + Y_i S^-1 Y_j^T,  [A^-1]_ij = (-K_i^T) .. (-K_{j-1}^T) [A^-1]_jj,  [A^-1]_jj = Sigma_jj - Y_j S^-1 Y_j^T
    if (JOINT) {
        const int npr = pp.counts[inst];
        const int32_t* pr = pp.pairs + (size_t)inst * pp.npair_max * 2;
        for (int p = tid; p < pp.npair_max; p += kAcThreads) {
            double* o = pp.cross + ((size_t)inst * pp.npair_max + p) * 36;
            const int pi = p < npr ? pr[2 * p] : -1, pj = p < npr ? pr[2 * p + 1] : -1;
            if (pi < 0 || pi >= nv || pj < 0 || pj >= nv || !ok) {   // an unused slot: 0; a singular window: NaN
                const double x = (p < npr && !ok) ? __builtin_nan("") : 0.0;
                for (int k = 0; k < 36; ++k) o[k] = x;
                continue;
            }
            const int lo = min(pi, pj), hi = max(pi, pj);
            double X[3][3];   // Sigma_{lo,hi}
            if (lo == hi) {
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        if (lo < nc) X[r][c] = (Hd[lo * 9 + r * 3 + c] + Hd[lo * 9 + c * 3 + r]) * 0.5;
                        else { const int b = 3 * (lo - nc); X[r][c] = (C[(b + r) * BS + b + c] + C[(b + c) * BS + b + r]) * 0.5; }
                    }
            } else if (lo >= nc) {
                const int bl = 3 * (lo - nc), bh = 3 * (hi - nc);
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c) X[r][c] = C[(bl + r) * BS + bh + c];
            } else if (hi >= nc) {
                const double* Yl = Ym + (size_t)lo * 3 * BS;
                const int bh = 3 * (hi - nc);
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c) X[r][c] = 0.0;
                for (int k = 0; k < D; ++k)
#pragma unroll
                    for (int r = 0; r < 3; ++r)
#pragma unroll
                        for (int c = 0; c < 3; ++c) X[r][c] = __builtin_fma(-Yl[r * BS + k], C[k * BS + bh + c], X[r][c]);
            } else {
                const double* Yl = Ym + (size_t)lo * 3 * BS;
                const double* Yh = Ym + (size_t)hi * 3 * BS;
                double hh[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, lh[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};   // Y_hi S^-1 Y_hi^T, Y_lo S^-1 Y_hi^T
                for (int q2 = 0; q2 < D; ++q2) {
                    double z[3] = {0, 0, 0};   // row q2 of S^-1 Y_hi^T
                    for (int k = 0; k < D; ++k)
#pragma unroll
                        for (int c = 0; c < 3; ++c) z[c] = __builtin_fma(C[q2 * BS + k], Yh[c * BS + k], z[c]);
#pragma unroll
                    for (int r = 0; r < 3; ++r)
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            hh[r][c] = __builtin_fma(Yh[r * BS + q2], z[c], hh[r][c]);
                            lh[r][c] = __builtin_fma(Yl[r * BS + q2], z[c], lh[r][c]);
                        }
                }
                double G[3][3];
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c) G[r][c] = (Hd[hi * 9 + r * 3 + c] + Hd[hi * 9 + c * 3 + r]) * 0.5 - hh[r][c];
                for (int k = hi - 1; k >= lo; --k) {   // (hi < nc <= nv_max: bounded by the window)
                    const double* K = Ho + k * 9;
                    double T[3][3];
#pragma unroll
                    for (int r = 0; r < 3; ++r)
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            double s2 = 0.0;
#pragma unroll
                            for (int t = 0; t < 3; ++t) s2 = __builtin_fma(K[t * 3 + r], G[t][c], s2);
                            T[r][c] = -s2;
                        }
#pragma unroll
                    for (int r = 0; r < 3; ++r)
#pragma unroll
                        for (int c = 0; c < 3; ++c) G[r][c] = T[r][c];
                }
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c) X[r][c] = G[r][c] + lh[r][c];
            }
            const bool tr = pi != lo;   // the pair was asked for as (hi, lo)
#pragma unroll
            for (int rr = 0; rr < 6; ++rr)
#pragma unroll
                for (int cc = 0; cc < 6; ++cc) {
                    double x = 0.0;
                    if (rr < 3 && cc < 3 && !((mk[pi] >> rr) & 1) && !((mk[pj] >> cc) & 1)) x = tr ? X[cc][rr] : X[rr][cc];
                    o[rr * 6 + cc] = x;
                }
        }
    }
}

template <int JAC, bool JOINT>
hipError_t launch_arrow_cov_j(const WindowArgs& a, double* ws, int cap, size_t lds, double* cov, int32_t* mask, int32_t* status, const CovPairs& pp, hipStream_t stream) {
    const hipError_t e = allow_dynamic_lds<&arrow_covariance_kernel<JAC, JOINT>>((int)kCovMaxLds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((arrow_covariance_kernel<JAC, JOINT>), dim3((unsigned)a.B), dim3(kAcThreads), lds, stream, a, ws, cap, cov, mask, status, pp);
    return hipGetLastError();
}
template <int JAC>
hipError_t launch_arrow_cov_t(const WindowArgs& a, double* ws, int cap, size_t lds, double* cov, int32_t* mask, int32_t* status, const CovPairs& pp, hipStream_t stream) {
    return pp.cross ? launch_arrow_cov_j<JAC, true>(a, ws, cap, lds, cov, mask, status, pp, stream) : launch_arrow_cov_j<JAC, false>(a, ws, cap, lds, cov, mask, status, pp, stream);
}

}  // namespace

size_t window_arrow_covariance_lds_bytes(const WindowCaps& c) { return arrow_cov_layout(c.nv_max).bytes; }
size_t window_arrow_covariance_workspace_doubles(const WindowCaps& c, int cap) { return arrow_cov_ws_doubles(c, cap); }

hipError_t launch_window_arrow_covariance(const WindowArgs& a, double* ws, int cap, double* cov, int32_t* mask, int32_t* status, const CovPairs& pp, hipStream_t stream) {
    if (a.B <= 0) return hipSuccess;
    if (!ws || cap < 1) return hipErrorInvalidValue;
    if (!cov_arrow_fits(a.caps)) return hipErrorInvalidValue;
    const size_t lds = arrow_cov_layout(a.caps.nv_max).bytes;
    return a.jacobian ? launch_arrow_cov_t<1>(a, ws, cap, lds, cov, mask, status, pp, stream) : launch_arrow_cov_t<0>(a, ws, cap, lds, cov, mask, status, pp, stream);
}

}  // namespace locamd
