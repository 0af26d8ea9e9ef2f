// What the reference reports of a window after a solve (loc_window_publish_resident, loc_window_path_resident, the node's loc_node_output;
// DESIGN.md §2, "Publish and path records of a resident batch"), stated once for the host and the device in message_rows.h's way: plain C++
// over one window — no HIP types, no allocation, no library call except sqrt.  It is Localization::publish() (localization.cpp:195-226: the
// gate of :199, Robot::current_pose() of robot.cpp:146-157, path->poses[trajectory_length / 2] of :220, tf::poseEigenToMsg's position and
// quaternion), Robot::vertices2path() (robot.cpp:61-72) and the destructor's tail path[T/2 .. T-1] (localization.cpp:708-717).
// window_publish_kernel.hip evaluates these functions one lane per record; frontend.cpp (the node) uses the same R_to_quat_xyzw and
// publish_gate; tests/host/pose_records_driver.cpp holds them to a numpy statement written from the reference's behaviour.
//
// The record arithmetic is sums, differences, one sqrt, one division and products of two factors: there is no multiply-add shape that
// contraction could fuse, and sqrt and / are the IEEE operations on both sides, so host and device produce the same bits.
//
// Conventions: a ring of T = trajectory_length poses of which a window holds the newest nv (slot 0 the oldest, slot nv - 1 the newest: both
// slides' and message_rows.h's convention).  Path index i of vertices2path's T poses is window slot i - (T - nv); the T - nv oldest ring
// vertices are the reference's never-measured initial vertices, which a window does not hold: they are reported as absent, not invented.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define LOCAMD_REC_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define LOCAMD_REC_HD inline
#endif

namespace locamd {

// Eigen::Quaterniond(R) (its four branches and their tie rules) then tf::poseEigenToMsg's w >= 0 flip; R row-major, out = (x, y, z, w)
LOCAMD_REC_HD void R_to_quat_xyzw(const double* R, double* q) {
    double w, x, y, z, t = R[0] + R[4] + R[8];
    if (t > 0) {
        t = sqrt(t + 1.0); w = 0.5 * t; t = 0.5 / t;
        x = (R[7] - R[5]) * t; y = (R[2] - R[6]) * t; z = (R[3] - R[1]) * t;
    } else if (R[0] >= R[4] && R[0] >= R[8]) {
        t = sqrt(R[0] - R[4] - R[8] + 1.0); x = 0.5 * t; t = 0.5 / t;
        w = (R[7] - R[5]) * t; y = (R[3] + R[1]) * t; z = (R[6] + R[2]) * t;
    } else if (R[4] > R[0] && R[4] >= R[8]) {
        t = sqrt(R[4] - R[8] - R[0] + 1.0); y = 0.5 * t; t = 0.5 / t;
        w = (R[2] - R[6]) * t; z = (R[7] + R[5]) * t; x = (R[1] + R[3]) * t;
    } else {
        t = sqrt(R[8] - R[0] - R[4] + 1.0); z = 0.5 * t; t = 0.5 / t;
        w = (R[3] - R[1]) * t; x = (R[2] + R[6]) * t; y = (R[5] + R[7]) * t;
    }
    if (w < 0) { w = -w; x = -x; y = -y; z = -z; }
    q[0] = x; q[1] = y; q[2] = z; q[3] = w;
}

// localization.cpp:199: strict.  A NaN chi2 compares false — not published, whatever the threshold (+inf included)
LOCAMD_REC_HD bool publish_gate(double chi2, double minimum_optimize_error) { return chi2 < minimum_optimize_error; }

// the window slot that holds path index i of a ring of T poses of which nv are in the window; negative: not in the window.  Slot nv - 1 is
// path index T - 1 (the newest pose)
LOCAMD_REC_HD int path_slot(int i, int nv, int T) { return i - (T - nv); }

// one pose (R row-major (9), t (3): the poses table's row) as position (3) + quaternion x, y, z, w (4)
LOCAMD_REC_HD void pose_record(const double* pose12, double* out7) {
    out7[0] = pose12[9]; out7[1] = pose12[10]; out7[2] = pose12[11];
    R_to_quat_xyzw(pose12, out7 + 3);
}

}  // namespace locamd
