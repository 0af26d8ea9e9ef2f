// gfx950 (MI355X / CDNA4): the newest pose and the factors of every resident window from ONE raw message per window
// (loc_window_message_rows_dev, loc_window_push_messages_resident_dev; DESIGN.md §2, "Rows from raw messages"): what Localization::addRangeEdge,
// Robot::new_vertex, addImuEdge, addLidarEdge and addTwistEdge do on the host for one node (localization.cpp:297-376, :438-535, :560-605;
// robot.cpp:75-110), for a whole batch on the device.  One launch writes exactly the arrays the two resident slides read: drop_oldest,
// new_pose, the three counts, new_r_idx / new_r_val, new_p_val, new_s_idx / new_s_val, and the verdict.
//
// Mapping: one wave per window, four windows per workgroup.  Every lane of a wave evaluates message_rows.h's rule on the same operands
// (wave-uniform arithmetic: a few hundred f64 operations, all in registers — the header's loops unroll to constant indices, the 6 x 6
// inversion included), and every lane keeps of each row the element it will store (LaneRows: one select per value, scalars only), so a 48-double
// EdgeSE3 row is one coalesced 384-byte store and not 48 stores of one lane.  No atomics, no LDS, no scratch, no dependence on
// the window's position in the batch; plain vector loads and stores only.
//
// It reads and writes nothing outside the handle's allocations and the caller's arrays:
//   * b = blockIdx.x * 4 + wave < B is tested first; every per-window array below is indexed by b alone and has B entries (rows).
//   * counts[b * 4]: the handle's [B][4] table.  x = poses[(b * nv_max + nv - 1) * 12 ..+12) is read only for 1 <= nv <= nv_max (the guard is
//     here, not only in the induction over the slides that keeps nv <= nv_max), inside window b's slice of the handle's [B][nv_max][12] array.
//   * the message arrays: kind[b], dt[b] always; anchor[b], antenna[b], distance[b], distance_err[b] only with LOC_MSG_RANGE in kinds_mask,
//     imu[b * 7 ..+7) with _IMU, lidar_z[b] with _LIDAR, twist[b * 42 ..+42) with _TWIST — the host has refused a NULL array under a mask bit —
//     and the values only under the same bit of kind[b], which message_rows() has then found inside the mask.
//   * anchors[anchor * 3 ..+3) after 0 <= anchor < n_anchors, antenna_xyz[(antenna - 1) * 3 ..+3) after 1 <= antenna <= n_antenna (both in
//     message_rows(): INVALID otherwise, before either is read).
//   * the outputs: drop_oldest[b], new_pose[b * 12 + lane] (lane < 12), the three counts [b], verdict[b] (when given); row e of new_r_idx /
//     new_r_val at (b * 2 + e) * 2 / * 5 for e < nr <= 2, of new_p_val at (b * 2 + e) * 18 for e < np <= 2, new_s_idx / new_s_val at b * 4 /
//     b * 48 for ns == 1: the capacities LOC_MSG_NR_NEW = 2, LOC_MSG_NP_NEW = 2, LOC_MSG_NS_NEW = 1 the arrays are declared with.  Rows at
//     or beyond a count (every row of a window whose verdict is not APPENDED) are left unwritten.
#include "message_rows.h"
#include "window_kernel.h"

namespace locamd {

namespace {

// message_rows()'s output as ONE lane of the wave sees it: of every array the element the lane will store (flat index == lane), the
// scalars as they are.  Scalars only: nothing here can end up in scratch.
struct LaneRows {
    int lane;
    int drop_oldest, nr, np, ns, verdict;
    double pose, r_val, p_val, s_val;
    int r_idx, s_idx;
    __device__ __forceinline__ void put_drop(int v) { drop_oldest = v; }
    __device__ __forceinline__ void put_pose(int k, double v) { pose = lane == k ? v : pose; }
    __device__ __forceinline__ void put_counts(int r, int p, int se3) { nr = r; np = p; ns = se3; }
    __device__ __forceinline__ void put_r_idx(int k, int v) { r_idx = lane == k ? v : r_idx; }
    __device__ __forceinline__ void put_r_val(int k, double v) { r_val = lane == k ? v : r_val; }
    __device__ __forceinline__ void put_p_val(int k, double v) { p_val = lane == k ? v : p_val; }
    __device__ __forceinline__ void put_s_idx(int k, int v) { s_idx = lane == k ? v : s_idx; }
    __device__ __forceinline__ void put_s_val(int k, double v) { s_val = lane == k ? v : s_val; }
    __device__ __forceinline__ void put_verdict(int v) { verdict = v; }
};

constexpr int kMsgWaves = 4;   // windows per workgroup

__global__ void __launch_bounds__(64 * kMsgWaves) window_message_kernel(const MessageArgs a) {
    const int lane = threadIdx.x & 63;
    const long long b = (long long)blockIdx.x * kMsgWaves + (threadIdx.x >> 6);
    if (b >= a.B) return;
    const int nv = a.counts[b * 4];
    const int nv_read = nv < a.nv_max ? nv : a.nv_max;
    const double* x = a.poses + ((size_t)b * a.nv_max + (nv_read >= 1 ? nv_read - 1 : 0)) * 12;   // (read by message_rows only when nv >= 1)
    const MessageConfig cfg{a.trajectory_length, a.maximum_velocity, a.distance_outlier, a.n_antenna, a.antenna_xyz};
    Message m{};
    m.kind = a.kind[b];
    m.dt = a.dt[b];
    if (a.kinds_mask & kMsgRange) { m.anchor = a.anchor[b]; m.antenna = a.antenna[b]; m.distance = a.distance[b]; m.distance_err = a.distance_err[b]; }
    if (a.kinds_mask & kMsgImu) m.imu = a.imu + (size_t)b * 7;
    if (a.kinds_mask & kMsgLidar) m.lidar_z = a.lidar_z[b];
    if (a.kinds_mask & kMsgTwist) m.twist = a.twist + (size_t)b * 42;
    LaneRows o{};
    o.lane = lane;
    message_rows(cfg, a.kinds_mask, nv, x, a.n_anchors, a.anchors, m, o);

    if (lane == 0) {
        a.drop_oldest[b] = o.drop_oldest;
        a.new_r_counts[b] = o.nr; a.new_p_counts[b] = o.np; a.new_s_counts[b] = o.ns;
        if (a.verdict) a.verdict[b] = o.verdict;
    }
    if (lane < 12) a.new_pose[(size_t)b * 12 + lane] = o.pose;
    // (the counts are -1 for every verdict but APPENDED: no row is stored)
    if (lane < o.nr * 2) a.new_r_idx[(size_t)b * kMsgNrNew * 2 + lane] = o.r_idx;
    if (lane < o.nr * 5) a.new_r_val[(size_t)b * kMsgNrNew * 5 + lane] = o.r_val;
    if (lane < o.np * 18) a.new_p_val[(size_t)b * kMsgNpNew * 18 + lane] = o.p_val;
    if (o.ns == 1) {
        if (lane < 4) a.new_s_idx[(size_t)b * kMsgNsNew * 4 + lane] = o.s_idx;
        if (lane < 48) a.new_s_val[(size_t)b * kMsgNsNew * 48 + lane] = o.s_val;
    }
}

}  // namespace

hipError_t launch_window_message_rows(const MessageArgs& a, hipStream_t stream) {
    if (a.B <= 0) return hipSuccess;
    if (!a.counts || !a.poses || !a.kind || !a.dt || a.nv_max <= 0 || (a.n_anchors > 0 && !a.anchors) || (a.n_antenna > 0 && !a.antenna_xyz)) return hipErrorInvalidValue;
    if ((a.kinds_mask & ~kMsgAllKinds) != 0) return hipErrorInvalidValue;
    if (((a.kinds_mask & kMsgRange) && (!a.anchor || !a.antenna || !a.distance || !a.distance_err)) || ((a.kinds_mask & kMsgImu) && !a.imu) ||
        ((a.kinds_mask & kMsgLidar) && !a.lidar_z) || ((a.kinds_mask & kMsgTwist) && !a.twist))
        return hipErrorInvalidValue;
    if (!a.drop_oldest || !a.new_pose || !a.new_r_counts || !a.new_r_idx || !a.new_r_val || !a.new_p_counts || !a.new_p_val || !a.new_s_counts || !a.new_s_idx || !a.new_s_val)
        return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((a.B + kMsgWaves - 1) / kMsgWaves);
    hipLaunchKernelGGL(window_message_kernel, dim3(blocks), dim3(64 * kMsgWaves), 0, stream, a);
    return hipGetLastError();
}

}  // namespace locamd
