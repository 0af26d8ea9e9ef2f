// Marginal covariance of one update's undamped normal matrix, shared by the COV variants of snapshot_lm_kernel and
// fusion_lm_kernel; covariance_kernel.hip shares the relative pivot threshold.  Internal to the including translation unit.
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>

namespace locamd {
namespace {

constexpr double kCovRelPivot = 1e-11;   // a pivot at most this fraction of its coordinate's diagonal entry of H is singular

__host__ __device__ __forceinline__ constexpr int cov_tri(int n, int r, int c) { return r * n - (r * (r - 1)) / 2 + (c - r); }

// h: the packed upper triangle (row-major: (0,0) (0,1) .. (0,N-1) (1,1) .. (N-1,N-1)) of H = sum J^T rho' Omega J.  On return h holds
// Sigma = H^-1 in the same packing, the exactly-zero-diagonal coordinates excluded (their rows / columns 0, their bits set in `mask`);
// false (and every entry NaN) if a pivot of H's LDL^T is not finite, not positive or at most kCovRelPivot of its diagonal entry.
// A tag without an active edge (every diagonal entry 0) gets every bit, zeros and true.
template <int N>
__device__ __forceinline__ bool cov_invert_packed(double (&h)[N * (N + 1) / 2], int& mask) {
    bool ex[N];
    double dg[N];
    mask = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        ex[i] = h[cov_tri(N, i, i)] == 0.0;   // H is a sum of J^T W J with W >= 0: its row and column are 0 as well
        mask |= ex[i] ? (1 << i) : 0;
    }
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int c = i; c < N; ++c) {
            const bool e = ex[i] || ex[c];
            h[cov_tri(N, i, c)] = e ? (c == i ? 1.0 : 0.0) : h[cov_tri(N, i, c)];
        }
#pragma unroll
    for (int i = 0; i < N; ++i) dg[i] = h[cov_tri(N, i, i)];
    // LDL^T, right-looking: row j of the packing becomes (1/d_j, l_{j+1,j} .. l_{N-1,j})
    bool ok = true;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const double d = h[cov_tri(N, j, j)];
        ok = ok && (d > kCovRelPivot * dg[j]) && (d < DBL_MAX);   // (NaN fails both)
        const double id = 1.0 / d;
#pragma unroll
        for (int i = j + 1; i < N; ++i)
#pragma unroll
            for (int c = i; c < N; ++c)
                h[cov_tri(N, i, c)] = __builtin_fma(-h[cov_tri(N, j, i)] * id, h[cov_tri(N, j, c)], h[cov_tri(N, i, c)]);
        h[cov_tri(N, j, j)] = id;
#pragma unroll
        for (int i = j + 1; i < N; ++i) h[cov_tri(N, j, i)] *= id;
    }
    // L^-1 (unit lower), column by column: m_ij = -(l_ij + sum_{j<k<i} l_ik m_kj), stored where l_ij was
#pragma unroll
    for (int j = 0; j < N; ++j)
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            double s = h[cov_tri(N, j, i)];
#pragma unroll
            for (int k = j + 1; k < i; ++k) s = __builtin_fma(h[cov_tri(N, k, i)], h[cov_tri(N, j, k)], s);
            h[cov_tri(N, j, i)] = -s;
        }
    // Sigma = L^-T D^-1 L^-1: Sigma_rc = sum_{k >= c} m_kr m_kc / d_k (m_kk = 1), row after row, each row left to right (in place: every
    // entry it overwrites is no longer read)
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
        for (int c = r; c < N; ++c) {
            double s = 0.0;
#pragma unroll
            for (int k = N - 1; k >= c; --k) {
                const double mkr = k == r ? 1.0 : h[cov_tri(N, r, k)];
                const double mkc = k == c ? 1.0 : h[cov_tri(N, c, k)];
                s = __builtin_fma(mkr * h[cov_tri(N, k, k)], mkc, s);
            }
            h[cov_tri(N, r, c)] = s;
        }
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
        for (int c = r; c < N; ++c) {
            const double v = (ex[r] || ex[c]) ? 0.0 : h[cov_tri(N, r, c)];
            h[cov_tri(N, r, c)] = ok ? v : __builtin_nan("");
        }
    return ok;
}

}  // namespace
}  // namespace locamd
