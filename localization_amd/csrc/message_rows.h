// The step that turns ONE raw message into the newest pose of ONE window and its factors (loc_window_message_rows_dev,
// loc_window_push_messages_resident_dev; DESIGN.md §2, "Rows from raw messages"), stated once for the host and the device in slide_admit.h's
// way: plain C++ over one window — no HIP types, no allocation, no library call except sin, cos, sqrt and fabs.  It is SURVEY §8(a) rows
// a5–a8, a10 and a11 of the reference: Localization::addRangeEdge (localization.cpp:297-376: the outlier gate, sigma^2, the two-edge topology,
// the antenna lever arm), Robot::new_vertex (robot.cpp:75-110: the initial estimate, drop-oldest), addImuEdge (:499-535), addLidarEdge
// (:462-496) and addTwistEdge with twist2transform / create_se3_edge_from_twist (:438-459, :560-605).  window_message_kernel.hip evaluates
// message_rows() wave-uniformly and spreads the stores over the lanes; frontend.cpp (the node) uses the same quat_to_R, iso_inverse, invert6
// and twist_transform; tests/host/message_rows_driver.cpp holds the function to a numpy statement written from the reference.
//
// All arithmetic is un-contracted (numeric_jacobian.h's idiom), every operation is an IEEE operation in the order written: host and device
// produce the same bits, except where sin and cos enter (the rotation of a TWIST row when the angular rate is not zero).
//
// With nv the window's count, x its newest solved pose (slot nv - 1), T = trajectory_length, drop = (nv == T) and s = nv - drop (the new slot):
//   drop_oldest = drop; new_pose = x (robot.cpp:90), then
//   RANGE   the frame-id branch of :327 is ALWAYS taken (every cfg/*.yaml stream takes it: consecutive range messages carry one frame id,
//           and the IMU / lidar ids are appended to it); the :348-350 branch (no requester vertex) is out of scope.
//           row 0: (s, -1 - anchor), measurement (double)distance, information 1 / ((double)distance_err)^2, lever arm antenna_xyz[antenna - 1],
//                  zeros for antenna == 0 (:331-336)
//           row 1: (s - 1, s), measurement 0, information 1 / (maximum_velocity dt / 3)^2, no lever arm (:338-340); left out when s == 0
//   IMU     first (:505-525): new_pose.R = quat_to_R(q) (not normalised), t kept; prior row Z^-1 = iso_inverse(new_pose), information
//           (0, 0, 0, 1/c0, 1/c4, 1/c8)
//   LIDAR   after IMU (:468-486): new_pose.t[2] = lidar_z; prior row Z^-1 = iso_inverse(new_pose), information (0, 0, 1/0.05, 0, 0, 0)
//   TWIST   (:438-459, :560-605) no range or prior row; one EdgeSE3 row (s - 1, s, 1, 0), Z^-1 = iso_inverse(twist_transform), information
//           invert6(cov dt^2)
//   gate    (:306-313) a RANGE message with distance_outlier > 0 and nv == T ("the window is at its lag": the batch's statement of
//           number_measurements > trajectory_length) is rejected when | ||x.t - anchor|| - (double)distance | > distance_outlier: vertex
//           origins only, no lever arm.
// dt is the message stamp minus the newest pose's stamp (:316, :442): the caller keeps the stamps.
//
// The verdict, by the FIRST test that decides, in this order (enum LOC_MSG_* of include/localization_amd.h):
//   NONE 0      kind == 0
//   INVALID 3   nv <= 0 or nv > T; a kind that is not RANGE with any subset of IMU / LIDAR or TWIST alone, or a bit outside kinds_mask; RANGE:
//               anchor outside [0, n_anchors), antenna outside [0, n_antenna]; TWIST with s == 0
//   REJECTED 2  the gate (as in the reference it comes before any covariance is formed)
//   INVALID 3   an information value that must be finite and positive and is not: 1 / distance_err^2, 1 / (maximum_velocity dt / 3)^2 (only
//               when row 1 exists), 1/c0, 1/c4, 1/c8.  STRICTER than the reference, which would hand g2o an infinity (distance_err == 0,
//               dt == 0, a zero IMU covariance) or a negative information.
//   SINGULAR 4  invert6 fails (a TWIST message with dt == 0 among them)
//   APPENDED 1
// For every verdict but APPENDED the three counts are -1 and no row is written; drop_oldest and new_pose are always written (new_pose = x;
// a window without poses has no x: the identity pose).  Rows beyond a count are never written.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define LOCAMD_MSG_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define LOCAMD_MSG_HD inline
#endif

namespace locamd {

#pragma clang fp contract(off)

struct Iso { double R[9]; double t[3]; };

LOCAMD_MSG_HD Iso iso_identity() { Iso x{}; x.R[0] = x.R[4] = x.R[8] = 1.0; return x; }
LOCAMD_MSG_HD Iso iso_inverse(const Iso& a) {
    Iso o;
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) o.R[i * 3 + j] = a.R[j * 3 + i];
    for (int i = 0; i < 3; ++i) o.t[i] = -(o.R[i * 3] * a.t[0] + o.R[i * 3 + 1] * a.t[1] + o.R[i * 3 + 2] * a.t[2]);
    return o;
}
// Eigen::Quaterniond(w,x,y,z).toRotationMatrix(), no normalisation (localization.cpp:509 relies on it)
LOCAMD_MSG_HD void quat_to_R(double w, double x, double y, double z, double* R) {
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}
// MatrixXd::inverse() of a 6x6 (partial pivoting); false if singular.  Every index is a compile-time constant once the loops are unrolled
// (the pivot row is exchanged by comparing r with p, not by indexing with p), so that the device keeps M in registers.
LOCAMD_MSG_HD bool invert6(const double* A, double* out) {
    double M[6][12];
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) { M[i][j] = A[i * 6 + j]; M[i][6 + j] = i == j ? 1.0 : 0.0; }
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        int p = c;
        double best = fabs(M[c][c]);
#pragma unroll
        for (int r = c + 1; r < 6; ++r) if (fabs(M[r][c]) > best) { p = r; best = fabs(M[r][c]); }
#pragma unroll
        for (int r = c + 1; r < 6; ++r)
            if (r == p) {
#pragma unroll
                for (int j = 0; j < 12; ++j) { const double v = M[c][j]; M[c][j] = M[r][j]; M[r][j] = v; }
            }
        const double d = M[c][c];
        if (d == 0.0 || !(fabs(d) <= 1.7976931348623157e308)) ok = false;   // (zero, infinite or NaN pivot)
        if (!ok) break;
#pragma unroll
        for (int j = 0; j < 12; ++j) M[c][j] /= d;
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            if (r == c || M[r][c] == 0.0) continue;
            const double f = M[r][c];
#pragma unroll
            for (int j = 0; j < 12; ++j) M[r][j] -= f * M[c][j];
        }
    }
    if (!ok) return false;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) out[i * 6 + j] = M[i][6 + j];
    return true;
}
// twist2transform (localization.cpp:560-583): tf::Quaternion::setRPY(wx dt, wy dt, wz dt), then tf::Matrix3x3::setRotation (normalising by
// 2 / |q|^2), translation v dt.  tw: linear (3), angular (3).
LOCAMD_MSG_HD Iso twist_transform(const double* tw, double dt) {
    const double hr = tw[3] * dt * 0.5, hp = tw[4] * dt * 0.5, hy = tw[5] * dt * 0.5;
    const double cy = cos(hy), sy = sin(hy), cp = cos(hp), sp = sin(hp), cr = cos(hr), sr = sin(hr);
    const double qx = sr * cp * cy - cr * sp * sy, qy = cr * sp * cy + sr * cp * sy, qz = cr * cp * sy - sr * sp * cy,
                 qw = cr * cp * cy + sr * sp * sy;
    const double s = 2.0 / (qx * qx + qy * qy + qz * qz + qw * qw);
    const double xs = qx * s, ys = qy * s, zs = qz * s;
    const double wx = qw * xs, wy = qw * ys, wz = qw * zs, xx = qx * xs, xy = qx * ys, xz = qx * zs, yy = qy * ys, yz = qy * zs, zz = qz * zs;
    Iso z;
    z.R[0] = 1.0 - (yy + zz); z.R[1] = xy - wz; z.R[2] = xz + wy;
    z.R[3] = xy + wz; z.R[4] = 1.0 - (xx + zz); z.R[5] = yz - wx;
    z.R[6] = xz - wy; z.R[7] = yz + wx; z.R[8] = 1.0 - (xx + yy);
    z.t[0] = tw[0] * dt; z.t[1] = tw[1] * dt; z.t[2] = tw[2] * dt;
    return z;
}

// ---- the rule ---------------------------------------------------------------------------------------------------------------------------------
enum MsgKind : int { kMsgRange = 1, kMsgImu = 2, kMsgLidar = 4, kMsgTwist = 8, kMsgAllKinds = 15 };
enum MsgVerdict : int { kMsgNone = 0, kMsgAppended = 1, kMsgRejected = 2, kMsgInvalid = 3, kMsgSingular = 4 };
enum : int { kMsgNrNew = 2, kMsgNpNew = 2, kMsgNsNew = 1 };   // the capacities of the rows one message makes (LOC_MSG_N*_NEW)

struct MessageConfig {
    int trajectory_length;
    double maximum_velocity;    // localization.cpp:319
    double distance_outlier;    // :78; <= 0: no gate
    int n_antenna;
    const double* antenna_xyz;  // [n_antenna][3] (:111-123); antenna is 1-based, 0 = none
};
// one window's message; an array is read only under its bit of `kind` (after `kind` is known to be legal and inside the mask)
struct Message {
    int kind;
    double dt;
    int anchor, antenna; float distance, distance_err;   // RANGE
    const double* imu;     // IMU [7]: q xyzw, orientation_covariance[0], [4], [8]
    double lidar_z;        // LIDAR
    const double* twist;   // TWIST [42]: linear 3, angular 3, covariance 36 row-major
};
// What one window gets, in the slides' layouts at the capacities kMsgN*New.  message_rows() hands every value to its `Out` argument through
// the eight calls below, each with the flat index of the value in the window's slice (row e of r_idx / r_val / p_val at e * 2 / e * 5 /
// e * 18).  This one keeps them in arrays (the host); window_message_kernel.hip's keeps, per lane, the one value the lane will store.
struct MessageRows {
    int drop_oldest;
    double new_pose[12];
    int nr, np, ns;
    int r_idx[kMsgNrNew * 2]; double r_val[kMsgNrNew * 5];
    double p_val[kMsgNpNew * 18];
    int s_idx[kMsgNsNew * 4]; double s_val[kMsgNsNew * 48];
    int verdict;
    void put_drop(int v) { drop_oldest = v; }
    void put_pose(int k, double v) { new_pose[k] = v; }
    void put_counts(int r, int p, int se3) { nr = r; np = p; ns = se3; }
    void put_r_idx(int k, int v) { r_idx[k] = v; }
    void put_r_val(int k, double v) { r_val[k] = v; }
    void put_p_val(int k, double v) { p_val[k] = v; }
    void put_s_idx(int k, int v) { s_idx[k] = v; }
    void put_s_val(int k, double v) { s_val[k] = v; }
    void put_verdict(int v) { verdict = v; }
};

LOCAMD_MSG_HD bool msg_information_ok(double v) { return v > 0.0 && v <= 1.7976931348623157e308; }

// one prior row on the new slot: Z^-1 = iso_inverse(pose), the information diagonal i0 .. i5
template <class Out>
LOCAMD_MSG_HD void msg_prior_row(Out& o, int row, const Iso& pose, double iz, double i3, double i4, double i5) {
    const Iso zi = iso_inverse(pose);
#pragma unroll
    for (int k = 0; k < 9; ++k) o.put_p_val(row * 18 + k, zi.R[k]);
#pragma unroll
    for (int k = 0; k < 3; ++k) o.put_p_val(row * 18 + 9 + k, zi.t[k]);
    o.put_p_val(row * 18 + 12, 0.0); o.put_p_val(row * 18 + 13, 0.0); o.put_p_val(row * 18 + 14, iz);
    o.put_p_val(row * 18 + 15, i3); o.put_p_val(row * 18 + 16, i4); o.put_p_val(row * 18 + 17, i5);
}

// nv: the window's count; x: its newest solved pose, [12] = R(9), t(3) (read only when nv >= 1); anchors: [n_anchors][3].
// Returns the verdict.  Nothing is put for a row at or beyond the counts.
template <class Out>
LOCAMD_MSG_HD int message_rows(const MessageConfig& cfg, int kinds_mask, int nv, const double* x, int n_anchors, const double* anchors, const Message& m, Out& o) {
    const int T = cfg.trajectory_length;
    const bool drop = nv == T;
    const int s = nv - (drop ? 1 : 0);
    Iso pose = iso_identity();
    if (nv >= 1) {
#pragma unroll
        for (int k = 0; k < 9; ++k) pose.R[k] = x[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) pose.t[k] = x[9 + k];
    }
    o.put_drop(drop ? 1 : 0);
    const int kind = m.kind;
    int verdict = kMsgAppended;
    const bool range = (kind & kMsgRange) != 0, imu = (kind & kMsgImu) != 0, lidar = (kind & kMsgLidar) != 0, twist = kind == kMsgTwist;
    if (kind == 0) verdict = kMsgNone;
    else if (nv <= 0 || nv > T) verdict = kMsgInvalid;
    else if ((kind & ~kinds_mask) != 0 || (kind & ~kMsgAllKinds) != 0 || !(twist || (range && (kind & kMsgTwist) == 0))) verdict = kMsgInvalid;
    else if (range && (m.anchor < 0 || m.anchor >= n_anchors || m.antenna < 0 || m.antenna > cfg.n_antenna)) verdict = kMsgInvalid;
    else if (twist && s == 0) verdict = kMsgInvalid;
    if (verdict == kMsgAppended && range && cfg.distance_outlier > 0.0 && drop) {   // :306-313, vertex origins
        const double* q = anchors + (size_t)m.anchor * 3;
        const double dx = pose.t[0] - q[0], dy = pose.t[1] - q[1], dz = pose.t[2] - q[2];
        const double distance_estimation = sqrt(dx * dx + dy * dy + dz * dz);
        if (fabs(distance_estimation - (double)m.distance) > cfg.distance_outlier) verdict = kMsgRejected;
    }
    int nr = -1, np = -1, ns = -1;
    if (verdict == kMsgAppended && range) {
        const double distance_cov = (double)m.distance_err * (double)m.distance_err;   // :318
        const double info0 = 1.0 / distance_cov;
        const double sd = cfg.maximum_velocity * m.dt / 3;                              // :319
        const double info1 = 1.0 / (sd * sd);
        double c0 = 1.0, c4 = 1.0, c8 = 1.0;
        if (imu) { c0 = 1.0 / m.imu[4]; c4 = 1.0 / m.imu[5]; c8 = 1.0 / m.imu[6]; }   // :516-518
        if (!msg_information_ok(info0) || (s > 0 && !msg_information_ok(info1)) || !msg_information_ok(c0) || !msg_information_ok(c4) || !msg_information_ok(c8))
            verdict = kMsgInvalid;
        else {
            nr = s > 0 ? 2 : 1; np = 0; ns = 0;
            o.put_r_idx(0, s); o.put_r_idx(1, -1 - m.anchor);
            o.put_r_val(0, (double)m.distance); o.put_r_val(1, info0);
#pragma unroll
            for (int k = 0; k < 3; ++k) o.put_r_val(2 + k, m.antenna > 0 ? cfg.antenna_xyz[(size_t)(m.antenna - 1) * 3 + k] : 0.0);   // :333-334
            if (s > 0) {
                o.put_r_idx(2, s - 1); o.put_r_idx(3, s);
                o.put_r_val(5, 0.0); o.put_r_val(6, info1); o.put_r_val(7, 0.0); o.put_r_val(8, 0.0); o.put_r_val(9, 0.0);
            }
            if (imu) {   // rotation overwritten, translation kept, :505-513
                quat_to_R(m.imu[3], m.imu[0], m.imu[1], m.imu[2], pose.R);
                msg_prior_row(o, np, pose, 0.0, c0, c4, c8);
                ++np;
            }
            if (lidar) {
                pose.t[2] = m.lidar_z;   // :474
                msg_prior_row(o, np, pose, 1 / 0.05, 0.0, 0.0, 0.0);   // :479
                ++np;
            }
        }
    }
    if (verdict == kMsgAppended && twist) {
        const Iso zi = iso_inverse(twist_transform(m.twist, m.dt));
        double cov[36], info[36];
#pragma unroll
        for (int i = 0; i < 36; ++i) cov[i] = m.twist[6 + i] * m.dt * m.dt;   // :579
        if (!invert6(cov, info)) verdict = kMsgSingular;
        else {
            nr = 0; np = 0; ns = 1;
            o.put_s_idx(0, s - 1); o.put_s_idx(1, s); o.put_s_idx(2, 1); o.put_s_idx(3, 0);   // robust: RobustKernelCauchy, :602
#pragma unroll
            for (int k = 0; k < 9; ++k) o.put_s_val(k, zi.R[k]);
#pragma unroll
            for (int k = 0; k < 3; ++k) o.put_s_val(9 + k, zi.t[k]);
#pragma unroll
            for (int k = 0; k < 36; ++k) o.put_s_val(12 + k, info[k]);
        }
    }
    // (pose is touched only after the last test that can refuse a RANGE message: new_pose of every other verdict is x)
#pragma unroll
    for (int k = 0; k < 9; ++k) o.put_pose(k, pose.R[k]);
#pragma unroll
    for (int k = 0; k < 3; ++k) o.put_pose(9 + k, pose.t[k]);
    o.put_counts(nr, np, ns);
    o.put_verdict(verdict);
    return verdict;
}

#pragma clang fp contract(fast)

}  // namespace locamd
