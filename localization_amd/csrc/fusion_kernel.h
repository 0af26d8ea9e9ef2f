// Internal interface of the 6-DoF fusion snapshot kernel (fusion_kernel.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace locamd {

struct FusionArgs {
    const float* dist;     // [K][2][B][4]
    const float* err;      // [K][2][B][4]
    const double* imu;     // [K][B][8]   q xyzw, orientation covariance c0 c4 c8, pad
    double* pose;          // [7][B]      state: t xyz, q xyzw (in/out)
    double* out_pose;      // [K][7][B]
    double* out_chi2;      // [K][B]
    uint8_t* out_trials;   // [K][B] or nullptr
    const double* anchors; // [8][3] device (padded rows 0)
    const double* offset;  // [3] device: antenna lever arm on the tag
    long long B;
    int K;
    int iterations;
    double gate;
    int gate_from_epoch;
    int jacobian;          // 0: analytic range Jacobians, 1: g2o's central differences (delta = 1e-9)
};

// The COV = true kernels' arguments: the solve's, plus each update's marginal covariance of the pose, SoA over tags.
// Coordinates: VertexSE3's minimal increment [dt (body), dq_xyz].
struct FusionCovArgs : FusionArgs {
    double* out_cov;          // [K][21][B]: row-major upper triangle of the 6x6 H^-1 (NaN when singular)
    int32_t* out_cov_mask;    // [K][B]: bits 0-5 = tx ty tz qx qy qz excluded (an exactly zero diagonal entry of H)
    int32_t* out_cov_status;  // [K][B]: LOC_OK or LOC_ERR_SINGULAR
};

hipError_t launch_fusion(const FusionArgs& a, int block_threads, hipStream_t stream);
// The same solve (bit for bit) with the covariance outputs as well; hipErrorInvalidValue if any of them is null.
hipError_t launch_fusion_cov(const FusionCovArgs& a, int block_threads, hipStream_t stream);

}  // namespace locamd
