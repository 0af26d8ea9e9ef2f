// gfx950 (MI355X / CDNA4): the reference's publish step and its path for a resident batch of windows (loc_window_publish_resident,
// loc_window_path_resident; DESIGN.md §2, "Publish and path records of a resident batch") — Localization::publish() (localization.cpp:195-226),
// Robot::vertices2path() (robot.cpp:61-72) and the destructor's tail (localization.cpp:708-717).  The rule is pose_records.h's, evaluated
// here per record; nothing of the batch is written.
//   window_publish_kernel, window b with nv = counts[b][0], chi2 = result[b][0], T = trajectory_length, ok = 1 <= nv <= T:
//     flags[b]      bit 0: ok and publish_gate(chi2, minimum_optimize_error); bit 1: ok and path_slot(T / 2, nv, T) >= 0 (whatever the gate says)
//     realtime[b]   pose_record(slot nv - 1), written only with bit 0
//     optimized[b]  pose_record(slot path_slot(T / 2, nv, T)), written only with bits 0 and 1
//     chi2[b]       result[b][0], always
//     n_published   += the windows with bit 0 (zeroed on the stream before the launch): every wave adds its ballot's population count with one
//                   vector atomic add — a sum of integers, the same whatever the order
//   window_path_kernel, window b and path index i = first + k, k < count: slot = path_slot(i, nv, T);
//     present[b][k] = ok and slot >= 0; path[b][k] = pose_record(slot), written only when present.  No gate: the reference has none there.
//
// Mapping: one lane per record — per window (publish), per (window, path index) (path).  A record is a gather of one 96-byte pose row and
// about 20 flops; consecutive lanes of the path kernel read consecutive rows of one window (unit stride), lanes of the publish kernel read
// rows nv_max * 96 bytes apart, each lane its own one or two cache lines, all of whose bytes it uses.  Blocks of one wave: the work is a
// handful of dependent loads per lane, so what hides their latency is the number of waves in flight across the CUs, not the block size.
// No LDS, no scratch, no barrier; every store is a vector store from the lane that owns the record; the grid is sized by the record count
// and the last wave is guarded.
#include "pose_records.h"
#include "window_kernel.h"

namespace locamd {

namespace {

constexpr int kPublishBlock = 64;

__device__ __forceinline__ void store_record(const double* pose, double* out) {
    double x[12], r[7];
#pragma unroll
    for (int i = 0; i < 12; ++i) x[i] = pose[i];
    pose_record(x, r);
#pragma unroll
    for (int i = 0; i < 7; ++i) out[i] = r[i];
}

__global__ void __launch_bounds__(kPublishBlock) window_publish_kernel(const PublishArgs a) {
    const long long b = (long long)blockIdx.x * kPublishBlock + threadIdx.x;
    const bool in = b < a.B;
    const int T = a.trajectory_length;
    const int nv = in ? a.counts[b * 4] : 0;
    const bool ok = in && nv >= 1 && nv <= T;   // (T <= nv_max: the host's check, so every slot below is inside the window's rows)
    double chi = 0.0;
    if (in) {
        chi = a.result[b * 8];
        if (a.chi2) a.chi2[b] = chi;
    }
    const bool pub = ok && publish_gate(chi, a.minimum_optimize_error);
    const int so = path_slot(T / 2, nv, T);
    const bool has_opt = ok && so >= 0;
    if (in) a.flags[b] = (pub ? 1 : 0) | (has_opt ? 2 : 0);
    if (pub) {
        const double* P = a.poses + (size_t)b * a.nv_max * 12;
        if (a.realtime) store_record(P + (size_t)(nv - 1) * 12, a.realtime + (size_t)b * 7);
        if (a.optimized && has_opt) store_record(P + (size_t)so * 12, a.optimized + (size_t)b * 7);
    }
    if (a.n_published) {   // (kernel argument: uniform)
        const int n = __popcll(__ballot(pub));
        if ((threadIdx.x & 63) == 0 && n) atomicAdd(a.n_published, n);
    }
}

__global__ void __launch_bounds__(kPublishBlock) window_path_kernel(const PathArgs a) {
    const long long g = (long long)blockIdx.x * kPublishBlock + threadIdx.x;
    if (g >= a.B * a.count) return;
    const long long b = g / a.count;
    const int k = (int)(g - b * a.count);
    const int T = a.trajectory_length;
    const int nv = a.counts[b * 4];
    const int slot = path_slot(a.first + k, nv, T);
    const bool present = nv >= 1 && nv <= T && slot >= 0;   // (first + k <= T - 1: slot <= nv - 1)
    a.present[g] = present ? 1 : 0;
    if (present) store_record(a.poses + ((size_t)b * a.nv_max + slot) * 12, a.path + (size_t)g * 7);
}

}  // namespace

hipError_t launch_window_publish(const PublishArgs& a, hipStream_t stream) {
    if (a.B <= 0) return hipSuccess;
    if (a.n_published) {
        const hipError_t e = hipMemsetAsync(a.n_published, 0, sizeof(int32_t), stream);
        if (e != hipSuccess) return e;
    }
    const long long blocks = (a.B + kPublishBlock - 1) / kPublishBlock;
    hipLaunchKernelGGL(window_publish_kernel, dim3((unsigned)blocks), dim3(kPublishBlock), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_window_path(const PathArgs& a, hipStream_t stream) {
    if (a.B <= 0 || a.count <= 0) return hipSuccess;
    const long long blocks = (a.B * a.count + kPublishBlock - 1) / kPublishBlock;
    hipLaunchKernelGGL(window_path_kernel, dim3((unsigned)blocks), dim3(kPublishBlock), 0, stream, a);
    return hipGetLastError();
}

}  // namespace locamd
