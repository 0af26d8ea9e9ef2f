// Stand-alone driver of tests/test_message_rows_cpu.py: localization_amd/csrc/message_rows.h (the rule window_message_kernel.hip evaluates) run
// window by window on the host, built with g++ under AddressSanitizer + UBSan with -ffp-contract=off and run as a program.  Every array a
// window's call may read is handed over in a heap block of EXACTLY its size (the pose only when nv >= 1, imu / twist only under their mask
// bit, the anchor and antenna tables at their counts), so a read beyond what the rule allows is a sanitizer report; the output arrays are
// poisoned before the call, so a row written beyond a count shows in the comparison.
//
//   message_rows_driver rows <in> <out>    the rule: a file of batches -> one record per window
//   message_rows_driver node <in> <out>    the node's host front end (frontend.cpp itself, compiled into this program with the solver
//                                          stubbed out: every publish flag is off, nothing is solved) fed one window's messages -> the
//                                          vertex and the edges every message added
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../localization_amd/csrc/frontend.cpp"   // (brings message_rows.h)

// ---- what frontend.cpp links against in the library: no device, no solve ---------------------------------------------------------------------------
static const char* g_last = "";
int locamd_fail(int code, const char* what) { g_last = what; return code; }
extern "C" {
int32_t loc_device_count(void) { return 1; }
int loc_window_create(loc_window**, int32_t, int64_t, const loc_window_caps*, int32_t, const double*, int32_t) { std::abort(); }
int loc_window_destroy(loc_window*) { std::abort(); }
int loc_window_set_anchors(loc_window*, int32_t, const double*) { std::abort(); }
int loc_window_set_jacobian(loc_window*, int32_t) { std::abort(); }
int loc_window_set_option(loc_window*, const char*, int64_t) { std::abort(); }
int loc_window_solve_host(loc_window*, int64_t, const int32_t*, double*, const int32_t*, const double*, const int32_t*, const double*, const int32_t*, const double*, double*) { std::abort(); }
int loc_window_last_kernel_ms(loc_window*, double*) { std::abort(); }
int loc_window_last_kernel_kind(const loc_window*, int32_t*) { std::abort(); }
}

namespace {

struct Reader {
    FILE* f;
    template <class T> T one() { T v; if (fread(&v, sizeof(T), 1, f) != 1) { fprintf(stderr, "short input\n"); exit(2); } return v; }
    // n values in a heap block of exactly n * sizeof(T) bytes (n == 0: a block of size 0 is never dereferenced)
    template <class T> std::unique_ptr<T[]> many(size_t n) {
        std::unique_ptr<T[]> p(new T[n]);
        if (n && fread(p.get(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
        return p;
    }
    bool more() { int c = fgetc(f); if (c == EOF) return false; ungetc(c, f); return true; }
};

constexpr int32_t kPoisonI = -77;
constexpr double kPoisonD = -7.77e77;

// one window's outputs, as tests/_message_rows_ref.py reads them back (RECORD)
struct Record {
    int32_t drop, nr, np, ns, verdict, r_idx[4], s_idx[4], pad;
    double pose[12], r_val[10], p_val[36], s_val[48];
};
static_assert(sizeof(Record) == 14 * 4 + 106 * 8, "Record is packed");

void poison(locamd::MessageRows& o) {
    o.drop_oldest = o.nr = o.np = o.ns = o.verdict = kPoisonI;
    for (int& v : o.r_idx) v = kPoisonI;
    for (int& v : o.s_idx) v = kPoisonI;
    for (double& v : o.new_pose) v = kPoisonD;
    for (double& v : o.r_val) v = kPoisonD;
    for (double& v : o.p_val) v = kPoisonD;
    for (double& v : o.s_val) v = kPoisonD;
}
void write_record(FILE* out, const locamd::MessageRows& o) {
    Record r{};
    r.drop = o.drop_oldest; r.nr = o.nr; r.np = o.np; r.ns = o.ns; r.verdict = o.verdict;
    std::memcpy(r.r_idx, o.r_idx, sizeof(r.r_idx)); std::memcpy(r.s_idx, o.s_idx, sizeof(r.s_idx));
    std::memcpy(r.pose, o.new_pose, sizeof(r.pose)); std::memcpy(r.r_val, o.r_val, sizeof(r.r_val));
    std::memcpy(r.p_val, o.p_val, sizeof(r.p_val)); std::memcpy(r.s_val, o.s_val, sizeof(r.s_val));
    fwrite(&r, sizeof(r), 1, out);
}

// a batch: int32 T, n_antenna, n_anchors, mask, B, pad; double vmax, outlier; antenna [n_antenna][3]; anchors [n_anchors][3]; then per window
// int32 nv, kind, anchor, antenna; float distance, distance_err; double dt, lidar_z; x [12] iff nv >= 1; imu [7] iff mask & 2; twist [42] iff mask & 8
int run_rows(const char* in, const char* outp) {
    Reader rd{fopen(in, "rb")};
    FILE* out = fopen(outp, "wb");
    if (!rd.f || !out) return 2;
    while (rd.more()) {
        const int32_t T = rd.one<int32_t>(), n_antenna = rd.one<int32_t>(), n_anchors = rd.one<int32_t>(), mask = rd.one<int32_t>(), B = rd.one<int32_t>();
        (void)rd.one<int32_t>();
        const double vmax = rd.one<double>(), outlier = rd.one<double>();
        const auto antenna = rd.many<double>((size_t)n_antenna * 3);
        const auto anchors = rd.many<double>((size_t)n_anchors * 3);
        const locamd::MessageConfig cfg{T, vmax, outlier, n_antenna, antenna.get()};
        for (int b = 0; b < B; ++b) {
            locamd::Message m{};
            const int32_t nv = rd.one<int32_t>();
            m.kind = rd.one<int32_t>(); m.anchor = rd.one<int32_t>(); m.antenna = rd.one<int32_t>();
            m.distance = rd.one<float>(); m.distance_err = rd.one<float>();
            m.dt = rd.one<double>(); m.lidar_z = rd.one<double>();
            const auto x = rd.many<double>(nv >= 1 ? 12 : 0);
            const auto imu = rd.many<double>((mask & 2) ? 7 : 0);
            const auto twist = rd.many<double>((mask & 8) ? 42 : 0);
            m.imu = (mask & 2) ? imu.get() : nullptr;
            m.twist = (mask & 8) ? twist.get() : nullptr;
            locamd::MessageRows o;
            poison(o);
            const int v = locamd::message_rows(cfg, mask, nv, nv >= 1 ? x.get() : nullptr, n_anchors, anchors.get(), m, o);
            if (v != o.verdict) { fprintf(stderr, "verdict returned %d, put %d\n", v, o.verdict); return 3; }
            write_record(out, o);
        }
    }
    fclose(out);
    return 0;
}

// the node: int32 T, n_antenna, n_anchors, n_msgs; double vmax, outlier; antenna; anchors; double start[3]; then per message
// int32 kind, anchor, antenna, pad; float distance, distance_err; double stamp, lidar_z; imu [7]; twist [42]
// Anchor a is node id 100 + a, the tag is id 200.  Per message one Record: what the message added, with the indices as flags (r_idx[0]: row 0
// is on the new vertex, r_idx[1]: -1 - the anchor's index, r_idx[2]: row 1 starts at the vertex before, r_idx[3]: and ends on the new one;
// s_idx likewise, [2]: robust); verdict = the call's return code.
int run_node(const char* in, const char* outp) {
    Reader rd{fopen(in, "rb")};
    FILE* out = fopen(outp, "wb");
    if (!rd.f || !out) return 2;
    const int32_t T = rd.one<int32_t>(), n_antenna = rd.one<int32_t>(), n_anchors = rd.one<int32_t>(), n_msgs = rd.one<int32_t>();
    const double vmax = rd.one<double>(), outlier = rd.one<double>();
    const auto antenna = rd.many<double>((size_t)n_antenna * 3);
    const auto anchors = rd.many<double>((size_t)n_anchors * 3);
    const auto start = rd.many<double>(3);
    loc_node_config cfg;
    loc_node_default_config(&cfg);
    cfg.trajectory_length = T; cfg.maximum_velocity = vmax; cfg.distance_outlier = outlier;   // (every publish_* flag is 0: no solve)
    std::vector<int32_t> ids;
    std::vector<double> pos(anchors.get(), anchors.get() + (size_t)n_anchors * 3);
    for (int a = 0; a < n_anchors; ++a) ids.push_back(100 + a);
    ids.push_back(200);
    pos.insert(pos.end(), start.get(), start.get() + 3);
    loc_node* n = nullptr;
    if (loc_node_create(&n, 0, &cfg, (int32_t)ids.size(), ids.data(), pos.data(), n_antenna, n_antenna ? antenna.get() : nullptr) != LOC_OK) { fprintf(stderr, "create: %s\n", g_last); return 3; }
    for (int k = 0; k < n_msgs; ++k) {
        const int32_t kind = rd.one<int32_t>(), anchor = rd.one<int32_t>(), ant = rd.one<int32_t>();
        (void)rd.one<int32_t>();
        const float distance = rd.one<float>(), distance_err = rd.one<float>();
        const double stamp = rd.one<double>(), lidar_z = rd.one<double>();
        const auto imu = rd.many<double>(7);
        const auto twist = rd.many<double>(42);
        RobotRing& r = *n->robot(200);
        const int last = r.last_vertex();
        const size_t nr0 = n->ranges.size(), np0 = n->priors.size(), ns0 = n->se3s.size();
        (void)nr0; (void)np0; (void)ns0;
        int rc = 0;
        locamd::MessageRows o;
        poison(o);
        o.nr = o.np = o.ns = 0;
        if (kind & 1) {
            rc = loc_node_add_range(n, 200, 100 + anchor, stamp, distance, distance_err, ant, "uwb", nullptr);
            if (kind & 2) {
                const double cov9[9] = {imu[4], 0, 0, 0, imu[5], 0, 0, 0, imu[6]};
                const int rc2 = loc_node_add_imu(n, stamp, imu.get(), cov9, "imu", nullptr);
                rc = rc ? rc : rc2;
                o.np += 1;
            }
            if (kind & 4) {
                const int rc2 = loc_node_add_lidar(n, stamp, lidar_z, "lidar", nullptr);
                rc = rc ? rc : rc2;
                o.np += 1;
            }
            o.nr = 2;
        } else if (kind & 8) {
            rc = loc_node_add_twist(n, stamp, twist.get(), twist.get() + 6, "uwb", nullptr);   // (the frame id of the range messages: the branch of :327 is then taken after a twist vertex too)
            o.ns = 1;
        }
        const int now = r.last_vertex();
        const Vertex& v = n->vertices.at(now);
        std::memcpy(o.new_pose, v.est.R, sizeof(double) * 9); std::memcpy(o.new_pose + 9, v.est.t, sizeof(double) * 3);
        for (int e = 0; e < o.nr; ++e) {
            const RangeEdge& x = n->ranges[n->ranges.size() - (size_t)o.nr + (size_t)e];
            if (e == 0) { o.r_idx[0] = x.v0 == now; o.r_idx[1] = -1 - (x.v1 - 100); }
            else { o.r_idx[2] = x.v0 == last; o.r_idx[3] = x.v1 == now; }
            double* d = o.r_val + e * 5;
            d[0] = x.meas; d[1] = x.info; d[2] = x.off[0]; d[3] = x.off[1]; d[4] = x.off[2];
        }
        for (int e = 0; e < o.np; ++e) {
            const PriorEdge& x = n->priors[n->priors.size() - (size_t)o.np + (size_t)e];
            if (x.v != now) { fprintf(stderr, "a prior that is not on the new vertex\n"); return 4; }
            double* d = o.p_val + e * 18;
            std::memcpy(d, x.zinv.R, sizeof(double) * 9); std::memcpy(d + 9, x.zinv.t, sizeof(double) * 3); std::memcpy(d + 12, x.info, sizeof(double) * 6);
        }
        if (o.ns) {
            const Se3Edge& x = n->se3s.back();
            o.s_idx[0] = x.vi == last; o.s_idx[1] = x.vj == now; o.s_idx[2] = x.robust; o.s_idx[3] = 0;
            std::memcpy(o.s_val, x.zinv.R, sizeof(double) * 9); std::memcpy(o.s_val + 9, x.zinv.t, sizeof(double) * 3); std::memcpy(o.s_val + 12, x.info, sizeof(double) * 36);
        }
        o.drop_oldest = 0;
        o.verdict = rc;
        write_record(out, o);
    }
    loc_node_destroy(n);
    fclose(out);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 4) { fprintf(stderr, "usage: message_rows_driver rows|node <in> <out>\n"); return 2; }
    if (!std::strcmp(argv[1], "rows")) return run_rows(argv[2], argv[3]);
    if (!std::strcmp(argv[1], "node")) return run_node(argv[2], argv[3]);
    return 2;
}
