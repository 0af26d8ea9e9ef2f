// A plain evaluator of the device functions the 6-DoF kernels share (device_math.h, window_device.h, se3_edge_device.h,
// cov_block_device.h, window_block_device.h): no reference and no comparison in here — tests/test_gpu_device_primitives.py holds both.
//   hipcc --offload-arch=gfx950 -O3 -I localization_amd/csrc tools/primitives_probe.hip -o tools/primitives_probe.bin
//   tools/primitives_probe.bin <op> <in.bin> <out.bin>
// in.bin: raw float64 rows of the op's input width; out.bin: raw float64 rows of its output width, one per input row.  The row
// formats are the Op structs below (NI doubles in, NO doubles out).  The wave / block reductions take one row per WAVE / BLOCK
// (64 / 64 NW values, one per lane) and write every lane's result.  Returns non-zero on any error.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include "cov_block_device.h"
#include "window_block_device.h"
using namespace locamd;

#define HIP_OK(call)                                                                                         \
    do {                                                                                                     \
        const hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess) {                                                                              \
            fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #call, hipGetErrorString(e_));            \
            return 3;                                                                                        \
        }                                                                                                    \
    } while (0)

// ---- one row per thread ----------------------------------------------------------------------------------------------------------------
struct OpMatToQuat { static constexpr int NI = 9, NO = 4; __device__ static void run(const double* in, double* out) { mat_to_quat(in, out); } };
struct OpMatToQuatRsq { static constexpr int NI = 9, NO = 4; __device__ static void run(const double* in, double* out) { mat_to_quat_rsq(in, out); } };
struct OpQuatNormalizeSign {   // q -> normalised q, the sign applied
    static constexpr int NI = 4, NO = 5;
    __device__ static void run(const double* in, double* out) {
        double q[4] = {in[0], in[1], in[2], in[3]};
        out[4] = quat_normalize_sign(q);
        for (int k = 0; k < 4; ++k) out[k] = q[k];
    }
};
struct OpQuatNormalizeSignRsq {
    static constexpr int NI = 4, NO = 4;
    __device__ static void run(const double* in, double* out) {
        double q[4] = {in[0], in[1], in[2], in[3]};
        quat_normalize_sign_rsq(q);
        for (int k = 0; k < 4; ++k) out[k] = q[k];
    }
};
struct OpQuatMul { static constexpr int NI = 8, NO = 4; __device__ static void run(const double* in, double* out) { quat_mul(in, in + 4, out); } };
struct OpQuatToMat { static constexpr int NI = 4, NO = 9; __device__ static void run(const double* in, double* out) { quat_to_mat(in, out); } };
struct OpQuatRightJac {   // q, sgn -> rows 3..5 x cols 3..5 of J (ldj = 6)
    static constexpr int NI = 5, NO = 9;
    __device__ static void run(const double* in, double* out) {
        double J[36];
        for (int k = 0; k < 36; ++k) J[k] = 0.0;
        quat_right_jac(in, in[4], J, 6);
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) out[r * 3 + c] = J[(3 + r) * 6 + 3 + c];
    }
};
// Xi (12: R row-major, t), Xj (12), the record (12: the inverse measurement, 36: the information matrix), robust, j_is_later ->
// chi, rterm, Hii (21), Hjj (21), Hoff (36), bi (6), bj (6); FULL = false writes chi and rterm only (the rest stays 0)
constexpr int kSe3In = 12 + 12 + 48 + 2, kSe3Out = 2 + 21 + 21 + 36 + 6 + 6;
template <bool FULL>
struct OpSe3 {
    static constexpr int NI = kSe3In, NO = kSe3Out;
    __device__ static void run(const double* in, double* out) {
        for (int k = 0; k < NO; ++k) out[k] = 0.0;
        double rterm = 0.0;
        out[0] = chain_se3_terms<FULL, 1>(in, in + 12, in + 24, in[72] != 0.0, in[73] != 0.0, out + 2, out + 23, out + 44, out + 80, out + 86, rterm);
        out[1] = rterm;
    }
};
struct OpPriorBlock { static constexpr int NI = 18 + 12, NO = 21; __device__ static void run(const double* in, double* out) { cov_prior_block(in, in + 18, out); } };
struct OpPriorBlockFull { static constexpr int NI = 12 + 36 + 12, NO = 21; __device__ static void run(const double* in, double* out) { cov_prior_block_full(in, in + 12, in + 48, out); } };
struct OpPriorBlock3 { static constexpr int NI = 12 + 36 + 12, NO = 6; __device__ static void run(const double* in, double* out) { cov_prior_block3(in, in + 12, in + 48, out); } };
struct OpPriorFullHessian { static constexpr int NI = 72, NO = 21; __device__ static void run(const double* in, double* out) { prior_full_hessian(in, in + 36, out); } };
struct OpPrior3MulAdd {   // w (6), e (3), acc (3) -> acc + W e
    static constexpr int NI = 12, NO = 3;
    __device__ static void run(const double* in, double* out) {
        for (int k = 0; k < 3; ++k) out[k] = in[9 + k];
        prior3_mul_add(in, in + 6, out);
    }
};
struct OpFastRcp { static constexpr int NI = 1, NO = 1; __device__ static void run(const double* in, double* out) { out[0] = fast_rcp(in[0]); } };
struct OpFastRcp1nr { static constexpr int NI = 1, NO = 1; __device__ static void run(const double* in, double* out) { out[0] = fast_rcp_1nr(in[0]); } };
struct OpSqrtAndRsqrt { static constexpr int NI = 1, NO = 2; __device__ static void run(const double* in, double* out) { sqrt_and_rsqrt(in[0], out[0], out[1]); } };
struct OpSqrtAndRsqrtFast { static constexpr int NI = 1, NO = 2; __device__ static void run(const double* in, double* out) { sqrt_and_rsqrt_fast(in[0], out[0], out[1]); } };
struct OpPivotRsqrt { static constexpr int NI = 1, NO = 1; __device__ static void run(const double* in, double* out) { out[0] = pivot_rsqrt(in[0]); } };
struct OpFastLogGe1 { static constexpr int NI = 1, NO = 1; __device__ static void run(const double* in, double* out) { out[0] = fast_log_ge1(in[0]); } };
struct OpFastLogGe1Scaled { static constexpr int NI = 2, NO = 1; __device__ static void run(const double* in, double* out) { out[0] = fast_log_ge1_scaled(in[0], (int)in[1]); } };

// ---- window_block_device.h: the 6x6 block steps of window_lm_kernel's factorisations ---------------------------------------------------------
// A matrix is 36 doubles ROW-major (its lower triangle is read); a factor is G (36, row-major, strict lower triangle) then ig (6); the
// blocks the products take are COLUMN-major, as the kernel stores them; a packed update is 27 doubles.
__device__ static void wbp_factor_in(const double* in, double (&G)[6][6], double (&ig)[6]) {
    for (int r = 0; r < 6; ++r) {
        for (int c = 0; c < 6; ++c) G[r][c] = in[6 * r + c];
        ig[r] = in[36 + r];
    }
}
// out: the lower triangle of G (row-major 36, the rest 0), ig (6), ok
__device__ static void wbp_factor_out(const double (&G)[6][6], const double (&ig)[6], bool ok, double* out) {
    for (int r = 0; r < 6; ++r) {
        for (int c = 0; c < 6; ++c) out[6 * r + c] = c <= r ? G[r][c] : 0.0;
        out[36 + r] = ig[r];
    }
    out[42] = ok ? 1.0 : 0.0;
}
template <bool IN_PLACE>
struct OpCholLeft {
    static constexpr int NI = 36, NO = 43;
    __device__ static void run(const double* in, double* out) {
        double G[6][6], ig[6];
        bool ok = true;
        if (IN_PLACE) {
            for (int r = 0; r < 6; ++r)
                for (int c = 0; c <= r; ++c) G[r][c] = in[6 * r + c];
            wb_chol_left([&](int r, int c) { return G[r][c]; }, G, ig, ok);
        } else wb_chol_left([&](int r, int c) { return in[6 * r + c]; }, G, ig, ok);
        wbp_factor_out(G, ig, ok, out);
    }
};
struct OpCholRight {   // (the diagonal of the output keeps the pivots)
    static constexpr int NI = 36, NO = 43;
    __device__ static void run(const double* in, double* out) {
        double A[6][6], ig[6];
        for (int r = 0; r < 6; ++r)
            for (int c = 0; c <= r; ++c) A[r][c] = in[6 * r + c];
        wb_chol_right(A, ig);
        wbp_factor_out(A, ig, wb_inverse_pivots_finite(ig), out);
    }
};
template <int FORM>   // G, ig, s -> x.  0: wb_forward_row, 1: wb_forward_row_scatter, 2: wb_back_solve_gather, 3: wb_back_solve_scatter,
struct OpRowSolve {   // 4: wb_back_solve_gather with the factor and the inverse pivots read where they lie (callable sources)
    static constexpr int NI = 48, NO = 6;
    __device__ static void run(const double* in, double* out) {
        double G[6][6], ig[6], s[6], x[6];
        wbp_factor_in(in, G, ig);
        for (int c = 0; c < 6; ++c) s[c] = x[c] = in[42 + c];
        if (FORM == 0) wb_forward_row(x, G, ig);
        else if (FORM == 1) wb_forward_row_scatter(x, G, ig);
        else if (FORM == 2) wb_back_solve_gather(s, G, ig, x);
        else if (FORM == 4) wb_back_solve_gather(s, [&](int s2, int rr) { return in[6 * s2 + rr]; }, [&](int rr) { return in[36 + rr]; }, x);
        else wb_back_solve_scatter(s, G, ig, x);
        for (int c = 0; c < 6; ++c) out[c] = x[c];
    }
};
template <bool LOAD>   // G, ig, row -> the block in memory (column-major 36, untouched entries 0) and its inverse pivots (6) after wb_store_factor_row
struct OpStoreFactorRow {   // of that row (a run-time index); LOAD: wb_load_factor of a block that holds G and ig, back as G (row-major) and ig
    static constexpr int NI = 43, NO = 42;
    __device__ static void run(const double* in, double* out) {
        double G[6][6], ig[6], mem[42];
        wbp_factor_in(in, G, ig);
        for (int k = 0; k < 42; ++k) mem[k] = 0.0;
        const int r = (int)in[42];
        if (!LOAD) wb_store_factor_row(r, G, ig, mem + r, 6, mem + 36 + r);
        else {
            double Gd[36], G2[6][6], ig2[6];
            for (int a = 0; a < 6; ++a)
                for (int b = 0; b < 6; ++b) { Gd[6 * b + a] = G[a][b]; G2[a][b] = 0.0; }
            wb_load_factor(Gd, ig, G2, ig2);
            for (int a = 0; a < 6; ++a) {
                for (int b = 0; b < 6; ++b) mem[6 * a + b] = G2[a][b];
                mem[36 + a] = ig2[a];
            }
        }
        for (int k = 0; k < 42; ++k) out[k] = mem[k];
    }
};
template <bool PACKED>   // B (column-major), y_K, then (!PACKED) G (row-major, lower), y -> G - lower(B B^T) (row-major, the rest 0), y - B y_K;
struct OpOuterLower {    // PACKED: -> the 27 sums as a packed update
    static constexpr int NI = PACKED ? 42 : 84, NO = PACKED ? 27 : 42;
    __device__ static void run(const double* in, double* out) {
        double B[36], yk[6];
        for (int k = 0; k < 36; ++k) B[k] = in[k];
        for (int k = 0; k < 6; ++k) yk[k] = in[36 + k];
        if (PACKED) wb_outer_lower(B, yk, [&](int r, int c, double v) { out[wb_tri(r, c)] = v; }, [&](int r, double v) { out[21 + r] = v; });
        else {
            double G[6][6], y[6];
            wbp_factor_in(in + 42, G, y);
            wb_outer_lower(B, yk, [&](int r, int c, double v) { G[r][c] -= v; }, [&](int r, double v) { y[r] -= v; });
            for (int r = 0; r < 6; ++r) {
                for (int c = 0; c < 6; ++c) out[6 * r + c] = c <= r ? G[r][c] : 0.0;
                out[36 + r] = y[r];
            }
        }
    }
};
struct OpBlockBlockTFms {   // Li, Lj, S (all column-major) -> S - Li Lj^T
    static constexpr int NI = 108, NO = 36;
    __device__ static void run(const double* in, double* out) {
        double S[36];
        for (int k = 0; k < 36; ++k) S[k] = in[72 + k];
        wb_block_blockT_fms(in, in + 36, S);
        for (int k = 0; k < 36; ++k) out[k] = S[k];
    }
};
template <bool FMS>   // B (column-major), x, t -> t - B^T x: wb_blockT_vec_sub / wb_blockT_vec_fms
struct OpBlockTVec {
    static constexpr int NI = 48, NO = 6;
    __device__ static void run(const double* in, double* out) {
        double x[6], t[6];
        for (int k = 0; k < 6; ++k) { x[k] = in[36 + k]; t[k] = in[42 + k]; }
        if (FMS) wb_blockT_vec_fms(in, x, t);
        else wb_blockT_vec_sub(in, x, t);
        for (int k = 0; k < 6; ++k) out[k] = t[k];
    }
};
struct OpDotFms { static constexpr int NI = 13, NO = 1; __device__ static void run(const double* in, double* out) { out[0] = wb_dot_fms(in, in + 6, in[12]); } };
struct OpRowBlockSub {   // li, B, S -> S - li B^T
    static constexpr int NI = 48, NO = 6;
    __device__ static void run(const double* in, double* out) {
        double li[6], S[6];
        for (int k = 0; k < 6; ++k) { li[k] = in[k]; S[k] = in[42 + k]; }
        wb_row_block_sub(li, in + 6, S);
        for (int k = 0; k < 6; ++k) out[k] = S[k];
    }
};
struct OpSubUpdate {   // G (row-major, lower), y, U -> G - U (row-major, lower, the rest 0), y - u
    static constexpr int NI = 69, NO = 42;
    __device__ static void run(const double* in, double* out) {
        double G[6][6], y[6];
        wbp_factor_in(in, G, y);
        wb_sub_update(G, y, in + 42);
        for (int r = 0; r < 6; ++r) {
            for (int c = 0; c < 6; ++c) out[6 * r + c] = c <= r ? G[r][c] : 0.0;
            out[36 + r] = y[r];
        }
    }
};

template <class Op>
__global__ void rows_kernel(const double* __restrict__ in, double* __restrict__ out, long long n) {
    const long long row = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (row >= n) return;
    double a[Op::NI], b[Op::NO];
    for (int k = 0; k < Op::NI; ++k) a[k] = in[row * Op::NI + k];
    Op::run(a, b);
    for (int k = 0; k < Op::NO; ++k) out[row * Op::NO + k] = b[k];
}

// chain_se3_terms<FULL, 64>: every lane's record is its column of an [entry][lane] LDS block, as chain_lm_kernel keeps it
template <bool FULL>
__global__ void __launch_bounds__(64) se3_vs64_kernel(const double* __restrict__ in, double* __restrict__ out, long long n) {
    __shared__ double blk[48 * 64];
    const int lane = threadIdx.x;
    const long long row = blockIdx.x * 64ll + lane;
    const bool live = row < n;
    double a[24 + 2], b[kSe3Out];
    for (int k = 0; k < kSe3Out; ++k) b[k] = 0.0;
    for (int k = 0; k < 48; ++k) blk[k * 64 + lane] = live ? in[row * kSe3In + 24 + k] : 0.0;
    if (live) {
        for (int k = 0; k < 24; ++k) a[k] = in[row * kSe3In + k];
        a[24] = in[row * kSe3In + 72]; a[25] = in[row * kSe3In + 73];
    }
    __syncthreads();
    if (!live) return;
    double rterm = 0.0;
    b[0] = chain_se3_terms<FULL, 64>(a, a + 12, blk + lane, a[24] != 0.0, a[25] != 0.0, b + 2, b + 23, b + 44, b + 80, b + 86, rterm);
    b[1] = rterm;
    for (int k = 0; k < kSe3Out; ++k) out[row * kSe3Out + k] = b[k];
}

// ---- one row per wave / block: every lane calls, every lane's result is written ----------------------------------------------------------
struct WvSum { __device__ static double run(double v) { return wave_sum(v); } };
struct WvMax { __device__ static double run(double v) { return wave_max(v); } };
struct WvPrev { __device__ static double run(double v) { return lane_from_prev(v); } };
struct WvNext { __device__ static double run(double v) { return lane_from_next(v); } };
template <class Op>
__global__ void __launch_bounds__(64) wave_kernel(const double* __restrict__ in, double* __restrict__ out) {
    const long long k = blockIdx.x * 64ll + threadIdx.x;
    out[k] = Op::run(in[k]);
}
template <int NW, int WHAT>   // 0: block_sum, 1: block_max, 2: block_any (input != 0 -> 1.0 / 0.0)
__global__ void __launch_bounds__(64 * NW) block_kernel(const double* __restrict__ in, double* __restrict__ out) {
    __shared__ double red[NW];
    const int tid = threadIdx.x;
    const long long k = blockIdx.x * (long long)(64 * NW) + tid;
    const double v = in[k];
    double r;
    if (WHAT == 0) r = block_sum<NW>(v, red, tid);
    else if (WHAT == 1) r = block_max<NW>(v, red, tid);
    else r = block_any<NW>(v != 0.0, red, tid) ? 1.0 : 0.0;
    out[k] = r;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
typedef void (*Launch)(const double* in, double* out, long long rows);
struct Entry { const char* name; int ni, no; Launch launch; };

template <class Op>
static void launch_rows(const double* in, double* out, long long n) {
    hipLaunchKernelGGL(rows_kernel<Op>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, 0, in, out, n);
}
template <bool FULL>
static void launch_se3_vs64(const double* in, double* out, long long n) {
    hipLaunchKernelGGL(se3_vs64_kernel<FULL>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, 0, in, out, n);
}
template <class Op>
static void launch_wave(const double* in, double* out, long long n) { hipLaunchKernelGGL(wave_kernel<Op>, dim3((unsigned)n), dim3(64), 0, 0, in, out); }
template <int NW, int WHAT>
static void launch_block(const double* in, double* out, long long n) {
    hipLaunchKernelGGL((block_kernel<NW, WHAT>), dim3((unsigned)n), dim3(64 * NW), 0, 0, in, out);
}
#define ROWS(name, Op) {name, Op::NI, Op::NO, launch_rows<Op>}
#define BLOCKS(name, WHAT) \
    {name "_1", 64, 64, launch_block<1, WHAT>}, {name "_2", 128, 128, launch_block<2, WHAT>}, \
    {name "_4", 256, 256, launch_block<4, WHAT>}, {name "_8", 512, 512, launch_block<8, WHAT>}
static const Entry kOps[] = {
    ROWS("mat_to_quat", OpMatToQuat), ROWS("mat_to_quat_rsq", OpMatToQuatRsq),
    ROWS("quat_normalize_sign", OpQuatNormalizeSign), ROWS("quat_normalize_sign_rsq", OpQuatNormalizeSignRsq),
    ROWS("quat_mul", OpQuatMul), ROWS("quat_to_mat", OpQuatToMat), ROWS("quat_right_jac", OpQuatRightJac),
    ROWS("se3_full_vs1", OpSe3<true>), ROWS("se3_chi_vs1", OpSe3<false>),
    {"se3_full_vs64", kSe3In, kSe3Out, launch_se3_vs64<true>}, {"se3_chi_vs64", kSe3In, kSe3Out, launch_se3_vs64<false>},
    ROWS("cov_prior_block", OpPriorBlock), ROWS("cov_prior_block_full", OpPriorBlockFull), ROWS("cov_prior_block3", OpPriorBlock3),
    ROWS("prior_full_hessian", OpPriorFullHessian), ROWS("prior3_mul_add", OpPrior3MulAdd),
    ROWS("fast_rcp", OpFastRcp), ROWS("fast_rcp_1nr", OpFastRcp1nr), ROWS("sqrt_and_rsqrt", OpSqrtAndRsqrt),
    ROWS("sqrt_and_rsqrt_fast", OpSqrtAndRsqrtFast), ROWS("pivot_rsqrt", OpPivotRsqrt),
    ROWS("fast_log_ge1", OpFastLogGe1), ROWS("fast_log_ge1_scaled", OpFastLogGe1Scaled),
    ROWS("wb_chol_left", OpCholLeft<false>), ROWS("wb_chol_left_in_place", OpCholLeft<true>), ROWS("wb_chol_right", OpCholRight),
    ROWS("wb_forward_row", OpRowSolve<0>), ROWS("wb_forward_row_scatter", OpRowSolve<1>),
    ROWS("wb_back_solve_gather", OpRowSolve<2>), ROWS("wb_back_solve_scatter", OpRowSolve<3>), ROWS("wb_back_solve_gather_in_place", OpRowSolve<4>),
    ROWS("wb_store_factor_row", OpStoreFactorRow<false>), ROWS("wb_load_factor", OpStoreFactorRow<true>),
    ROWS("wb_dot_fms", OpDotFms), ROWS("wb_row_block_sub", OpRowBlockSub), ROWS("wb_sub_update", OpSubUpdate),
    ROWS("wb_outer_lower_sub", OpOuterLower<false>), ROWS("wb_outer_lower_packed", OpOuterLower<true>),
    ROWS("wb_block_blockT_fms", OpBlockBlockTFms), ROWS("wb_blockT_vec_sub", OpBlockTVec<false>), ROWS("wb_blockT_vec_fms", OpBlockTVec<true>),
    {"wave_sum", 64, 64, launch_wave<WvSum>}, {"wave_max", 64, 64, launch_wave<WvMax>},
    {"lane_from_prev", 64, 64, launch_wave<WvPrev>}, {"lane_from_next", 64, 64, launch_wave<WvNext>},
    BLOCKS("block_sum", 0), BLOCKS("block_max", 1), BLOCKS("block_any", 2),
};

int main(int argc, char** argv) {
    if (argc != 4) {
        fprintf(stderr, "usage: %s <op> <in.bin> <out.bin>\nops:", argv[0]);
        for (const Entry& e : kOps) fprintf(stderr, " %s(%d->%d)", e.name, e.ni, e.no);
        fprintf(stderr, "\n");
        return 1;
    }
    const Entry* op = nullptr;
    for (const Entry& e : kOps)
        if (!strcmp(e.name, argv[1])) op = &e;
    if (!op) { fprintf(stderr, "unknown op %s\n", argv[1]); return 1; }
    FILE* f = fopen(argv[2], "rb");
    if (!f) { perror(argv[2]); return 1; }
    std::vector<double> in;
    double buf[4096];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) {
        if (got % sizeof(double)) { fprintf(stderr, "%s: not a whole number of doubles\n", argv[2]); fclose(f); return 1; }
        in.insert(in.end(), buf, buf + got / sizeof(double));
    }
    fclose(f);
    if (in.empty() || in.size() % (size_t)op->ni) { fprintf(stderr, "%s: %zu doubles are not rows of %d\n", argv[2], in.size(), op->ni); return 1; }
    const long long n = (long long)(in.size() / (size_t)op->ni);
    if (n > (1ll << 24)) { fprintf(stderr, "too many rows\n"); return 1; }
    std::vector<double> out((size_t)n * op->no, 0.0);
    double *din = nullptr, *dout = nullptr;
    HIP_OK(hipMalloc((void**)&din, in.size() * sizeof(double)));
    HIP_OK(hipMalloc((void**)&dout, out.size() * sizeof(double)));
    HIP_OK(hipMemcpy(din, in.data(), in.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_OK(hipMemset(dout, 0, out.size() * sizeof(double)));
    op->launch(din, dout, n);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(out.data(), dout, out.size() * sizeof(double), hipMemcpyDeviceToHost));
    HIP_OK(hipFree(din));
    HIP_OK(hipFree(dout));
    f = fopen(argv[3], "wb");
    if (!f) { perror(argv[3]); return 1; }
    const bool ok = fwrite(out.data(), sizeof(double), out.size(), f) == out.size();
    if (fclose(f) != 0 || !ok) { fprintf(stderr, "%s: short write\n", argv[3]); return 1; }
    return 0;
}
