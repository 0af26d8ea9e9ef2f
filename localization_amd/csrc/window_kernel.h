// Internal interface of the sliding-window graph solver kernel (window_kernel.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

namespace locamd {

// Host side of every launch that asks for more than 64 KiB of dynamic LDS: the opt-in is per device and per kernel (instantiation), so
// each instantiation of this helper keeps one flag word, a bit per device, and asks the runtime once.
template <auto Kernel>
inline hipError_t allow_dynamic_lds(int bytes) {
    static std::atomic<uint64_t> attr_set{0};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const uint64_t bit = 1ull << (dev & 63);
    if (attr_set.load(std::memory_order_acquire) & bit) return hipSuccess;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) attr_set.fetch_or(bit, std::memory_order_release);
    return e;
}

// Per-batch capacities; every instance owns fixed-size slices of the arrays below.
struct WindowCaps {
    int nv_max;  // moving poses per instance
    int nr_max;  // range edges
    int np_max;  // unary SE3 priors
    int ns_max;  // binary SE3 edges   (edge tables and records must fit 160 KiB of LDS)
    int bw_max;  // widest coupling between poses of one instance, in pose slots (|vi - vj| of any binary edge)
};

// Layout of one instance (all arrays are [B][...]):
//   counts  int32 [B][4]            nv, nr, np, ns
//   poses   double[B][nv_max][12]   R row-major (9), t (3)            in: estimate, out: optimised
//   r_idx   int32 [B][nr_max][2]    v0 (moving slot), v1 (moving slot, or -1 - anchor index)
//   r_val   double[B][nr_max][5]    measurement, information, lever arm of endpoint 0 (xyz)
//   p_idx   int32 [B][np_max]       v
//   p_val   double[B][np_max][18]   Z^-1 as R(9), t(3); information diagonal (6)
//   s_idx   int32 [B][ns_max][4]    vi, vj, robust, pad
//   s_val   double[B][ns_max][48]   Z^-1 as R(9), t(3); information 6x6 row-major (36)
//   result  double[B][8]            chi2 (all edges, last evaluated), robust chi2, lambda, outer iterations,
//                                   LM trials, terminated, number of binary edges that share their pair of poses with another edge,
//                                   (nv_max <= 512) elimination-tree levels * 65536 + blocks of the factor + root-supernode poses / 16
struct WindowArgs {
    const int32_t* counts;
    const double* poses_in;  // initial estimates (may alias `poses`: every instance reads its poses before it writes them)
    double* poses;           // optimised estimates
    const int32_t* r_idx; const double* r_val;
    const double* r_off1;   // optional [B][nr_max][3]: lever arm of endpoint 1 (types_edge_se3range.h:73 offset[1]); nullptr = none (general kernel only)
    const int32_t* p_idx; const double* p_val;
    const double* p_info;   // optional [B][np_max][36]: full information matrix of every prior, row-major, in the place of p_val's diagonal; nullptr = none (general kernel, envelope covariance pass, marginal prior pass)
    const int32_t* s_idx; const double* s_val;
    const double* anchors;  // [n_anchors][3] fixed vertices (identity rotation), shared by all instances
    double* result;
    double* workspace;  // nullptr: skyline H/L in LDS; else [B][window_workspace_doubles] in HBM (large windows)
    int n_anchors;
    int B;
    int iterations;
    int jacobian;       // 0: analytic range Jacobians, 1: g2o's central differences (delta = 1e-9)
    int natural_order;  // != 0: windows of <= 512 poses are eliminated in the caller's pose order (diagnostics / tests)
    WindowCaps caps;
};

size_t window_lds_bytes(const WindowCaps& c, bool global_a);
size_t window_workspace_doubles(const WindowCaps& c);
hipError_t launch_window(const WindowArgs& a, hipStream_t stream);
// chain windows, one lane per window (window_kernel.hip: chain_lm_kernel): workspace size in doubles, launch
size_t window_chain_workspace_doubles(const WindowCaps& c, long long B);
hipError_t launch_window_chain(const WindowArgs& a, double* chain_ws, hipStream_t stream);

// translation-only chain windows, one lane per window (chain3_kernel.hip)
size_t window_chain3_workspace_doubles(const WindowCaps& c, long long B);
int window_chain3_lds_mode(const WindowCaps& c, long long B, int n_cus);   // bit 0: (G, y) in LDS, bit 1: the translations in LDS
hipError_t launch_window_chain3(const WindowArgs& a, double* ws, hipStream_t stream);

// translation-only chain windows of <= 64 poses, one wave per window (wave3_kernel.hip): the node's own solve, small batches
// pinfo: with the prior records of wave3_lm_kernel<JAC, true> (a.p_info set: a dense 3 x 3 information block per prior)
size_t window_wave3_lds_bytes(const WindowCaps& c, bool pinfo = false);
hipError_t launch_window_wave3(const WindowArgs& a, hipStream_t stream);

// 6-DoF chain windows of <= 64 poses without EdgeSE3 factors and with at most one range edge per pair of consecutive poses, one wave
// per window (wave6_kernel.hip): the node's own solve with IMU priors / lever arms, small batches
size_t window_wave6_lds_bytes(const WindowCaps& c, bool se3 = false);   // se3: with the EdgeSE3 records of wave6_lm_kernel<JAC, true> (an EdgeSE3 per consecutive pair)
hipError_t launch_window_wave6(const WindowArgs& a, bool se3, hipStream_t stream);

// translation-only chain + dense border windows (arrow3_kernel.hip): four waves per window.  The host cuts the chain into up to
// four segments at separator poses (which join the border), orders the rows (chain rows by segment, then border rows) and packs
// every row's edges and priors as records [chunk of 64 rows][slot][lane] once per upload (capi_window.cpp: build_arrow_aux).
constexpr int kArrowMaxAnchors = 256;   // fixed anchors an edge of such a window may name: the table is staged in LDS (6 KB)
struct ArrowAux {
    const int32_t* hdr;     // [B][8]  nb (border poses incl. separators), nseg, n (chain rows), seg[0 .. 4] (chain rows of segment s: [seg[s], seg[s+1]))
    const int32_t* rslot;   // [B][nv_max] pose slot of row r (rows 0 .. n-1: chain, n .. n+nb-1: border)
    const double* rec;      // [B][nchunk][jmax][64][3]  code, measurement, information; code < 0: none; else (index << 3) | (kind << 1) | own-is-endpoint-0,
                            //                           kind 0: fixed anchor `index`, 1: the previous chain row, 2: border pose `index`
    const double* prec;     // [B][nchunk][jpmax][64][7] flag (> 0: a prior), Z^-1.t (3), information diagonal (3)
    double* ws;             // [B][window_arrow3_workspace_doubles]
    int nb_max, jmax, jpmax, nchunk;
    int jch[16], jpch[16];  // per chunk of 64 rows: the most edge / prior records any of its rows has, over the batch (<= jmax, jpmax; chunks from 16 on: jmax, jpmax)
};
size_t window_arrow3_workspace_doubles(const WindowCaps& c, int nb_max);
size_t window_arrow3_lds_bytes(const WindowCaps& c, int nb_max);
hipError_t launch_window_arrow3(const WindowArgs& a, const ArrowAux& x, hipStream_t stream);

// forest windows of ONE shared topology, one lane per window (tree_kernel.hip: tree_lm_kernel) or one wave per window (tree_wave_kernel.hip): the elimination schedule the
// host builds once per upload (capi_window.cpp: build_tree_sched); all pointers are device arrays shared by the whole batch
struct TreeSched {
    const int32_t* node;    // [nv]   pose slot of the k-th node in elimination order (children before their parent)
    const int32_t* par;     // [nv]   position (in that order) of the node's parent, -1 for a root
    const int32_t* r_off;   // [nv+1] the node's range edges (to anchors, or to its parent) = r_list[r_off[k] .. r_off[k+1])
    const int32_t* r_list;  // [nr]   edge numbers in schedule order (the kernel copies the values into its workspace in this order)
    const int32_t* p_off; const int32_t* p_list;   // priors of the node
    const int32_t* s_off; const int32_t* s_list;   // EdgeSE3 factors between the node and its parent
    const int32_t* r_idx;   // [nr][2], [ns][4]: the index tables of instance 0 (= of every instance); tree_wave_kernel<JAC, TreeGroups> points its wave's copy at the window's own rows
    const int32_t* s_idx;
    // the same structure by POSE SLOT, for tree_wave_kernel (one wave per window, lane = pose): parent slot (-1: root), height above
    // the leaves, children (w_klist[w_koff[v] .. w_koff[v+1])), and the edges of the pose (unary ones, and those to its parent)
    const int32_t *w_par, *w_height, *w_koff, *w_klist, *w_roff, *w_rlist, *w_poff, *w_plist, *w_soff, *w_slist;
    const int32_t* w_kleaf;   // [nv] how many of a pose's children are leaves (they come first in w_klist)
    const int32_t* w_ulist;   // [nu] the inner nodes (height >= 1) by pose slot, PARENTS FIRST (decreasing height)
    const int32_t* w_kpos;    // [nv] a pose's position in w_klist (= the LDS column its hand-over to the parent uses: a node's children are
                              //      consecutive columns); roots: nv - nroots, nv - nroots + 1, ...
    int nv, nr, np, ns, depth, nroots, nlev, max_se3_per_node, nu, max_r_per_node;
};
// Forest windows of DIFFERING topologies (option "forest_groups"; window_structure.cpp: build_tree_groups): one schedule per group of windows
// of one topology, one device block [hdr | sched_of | pad | tables].  hdr: kTreeGroupHdr int32 per group — TreeSched's ten sizes in their
// declaration order, the offset of the group's table in `tables` (int32s, a multiple of 4), the table's length.  A group's table is
// build_tree_sched's, bound by tree_sched_bind (window_layouts.h) on the host and in the kernel alike; its r_idx / s_idx sections hold the
// group's FIRST window's rows — the twin kernel reads every window's own rows (anchor numbers and robust flags are not part of a topology).
constexpr int kTreeGroupHdr = 12;
constexpr int32_t kTreeGroupPoison = INT32_MIN;   // the padding between sched_of and the tables, and behind every table up to a multiple of 4
struct TreeGroups {
    const int32_t* hdr;        // [n_groups][kTreeGroupHdr]
    const int32_t* sched_of;   // [B] window -> group
    const int32_t* tables;     // the groups' tables, concatenated
    int n_groups;
};
// The pose pairs of a joint covariance call (loc_window_joint_covariance_*), device arrays.  cross == nullptr: the plain call
// (the passes' kernels without any pair code).  Otherwise every pass also writes cross[b][p] = [H^-1]_ij for the pairs p < counts[b] of
// window b (6x6 row-major, rows: pose i; excluded rows / columns 0; NaN for a singular window) and 0 for the slots p >= counts[b].  The
// host has checked every slot (window_structure.cpp: check_pairs).
struct CovPairs {
    const int32_t* counts;   // [B]
    const int32_t* pairs;    // [B][npair_max][2]  pose slots i, j
    double* cross;           // [B][npair_max][36]
    int npair_max;
};

// marginal pose covariances of chain windows of <= 64 poses at a.poses (covariance_kernel.hip): one wave per window, 3x3 blocks for
// translation-only batches (d3), 6x6 otherwise; cov [B][nv_max][36], mask [B][nv_max], status [B] (device arrays)
size_t window_covariance_lds_bytes(const WindowCaps& c, bool d3);
hipError_t launch_window_covariance(const WindowArgs& a, bool d3, double* cov, int32_t* mask, int32_t* status, const CovPairs& pp, hipStream_t stream);

// the same for forest windows of ONE shared topology of <= 64 poses (forest_covariance_kernel.hip): one wave per window on the solve
// kernels' elimination schedule, always 6x6 blocks
size_t window_forest_covariance_lds_bytes(const TreeSched& ts);
hipError_t launch_window_forest_covariance(const WindowArgs& a, const TreeSched& ts, double* cov, int32_t* mask, int32_t* status, const CovPairs& pp, hipStream_t stream);
// the same for forest windows of DIFFERING topologies (option "forest_groups_covariance"; forest_covariance_groups_kernel.hip): every wave walks
// the schedule of its window's group.  host_hdr: the host's copy of g.hdr, whose sizes are checked before the launch
hipError_t launch_window_forest_covariance_groups(const WindowArgs& a, const TreeGroups& g, const int32_t* host_hdr, double* cov, int32_t* mask, int32_t* status,
                                                  const CovPairs& pp, hipStream_t stream);

// the same for translation-only arrowhead windows (arrow_covariance_kernel.hip: the windows arrow3_lm_kernel solves; border = the last slots
// by build_arrow_aux's rule, recomputed on the device), one workgroup per window, 3x3 blocks.  ws: [B][window_arrow_covariance_workspace_doubles]
// in HBM (edge records, B, Y = A^-1 B and a list of `cap` edges per pose); cap: the most edges and priors any pose in front of the border has
size_t window_arrow_covariance_lds_bytes(const WindowCaps& c);
size_t window_arrow_covariance_workspace_doubles(const WindowCaps& c, int cap);
hipError_t launch_window_arrow_covariance(const WindowArgs& a, double* ws, int cap, double* cov, int32_t* mask, int32_t* status, const CovPairs& pp, hipStream_t stream);

// the same for windows of any structure and length (envelope_covariance_kernel.hip: what the three passes above decline), one workgroup per
// window, 6x6 blocks, block LDL^T and selected inversion on the envelope of the caller's pose order.  blocks: the batch's largest envelope
// (window_structure.cpp: envelope_blocks_max); ws: [B][window_envelope_covariance_workspace_doubles] in HBM (the envelope, one column, diag(H))
size_t window_envelope_covariance_lds_bytes(const WindowCaps& c);
size_t window_envelope_covariance_workspace_doubles(const WindowCaps& c, long long blocks);
hipError_t launch_window_envelope_covariance(const WindowArgs& a, double* ws, long long blocks, double* cov, int32_t* mask, int32_t* status, const CovPairs& pp, hipStream_t stream);

// the marginal prior a dropped pose leaves on its one neighbour, translation-only windows (marginal_prior_kernel.hip): one wave
// per window at a.poses; drop [B] (checked on the host: window_structure.cpp, check_marginal_drop), slot [B], prior [B][48], grad / shift
// [B][6], rank / status [B] (device arrays)
hipError_t launch_window_marginal_prior(const WindowArgs& a, const int32_t* drop, int32_t* slot, double* prior, double* grad, double* shift, int32_t* rank, int32_t* status,
                                        hipStream_t stream);

// the resident slide's re-pack (window_slide_kernel.hip; DESIGN.md §2, "The resident slide"): one wave per window, in place on the resident
// batch's tables, after launch_window_marginal_prior has left the marginal of slot 0 in m_*.  All device arrays; the host has admitted
// every count and index (window_structure.cpp: slide_indices).
struct SlideArgs {
    int32_t* counts; double* poses; double* poses_in;   // [B][4]; the optimised estimates x (read, then re-packed); the next solve's input estimates
    int32_t* r_idx; double* r_val; int32_t* p_idx; double* p_val; double* p_info;
    const int32_t* drop;                                 // [B] != 0: the window drops slot 0
    const double* new_pose;                              // [B][12]
    const int32_t* new_r_counts; const int32_t* new_r_idx; const double* new_r_val;   // [B], [B][nr_new_max][2], [B][nr_new_max][5]
    const int32_t* new_p_counts; const double* new_p_val;                             // [B], [B][np_new_max][18]
    const int32_t* m_slot; const double* m_prior; const int32_t* m_rank; const int32_t* m_status;   // the marginal pass's results
    int32_t* slot; double* prior; int32_t* rank; int32_t* status;                     // the caller's outputs, each may be nullptr
    int nr_new_max, np_new_max, B;
    WindowCaps caps;
};
// densify: p_info is a NEW table (the handle had none): every row but the carried one becomes diag(p_val[12..17])
hipError_t launch_window_slide(const SlideArgs& s, bool densify, hipStream_t stream);
// the twin of loc_window_slide_resident_dev: the host has admitted NOTHING.  drop (may be nullptr: every window drops), new_pose and the new
// rows are the caller's device arrays; each wave admits its own window against slide_admit.h's rule (new anchor codes against n_anchors),
// writes admit[b] (may be nullptr) and either re-packs as above or reports slot -1, 48 zeros, rank 0, status LOC_ERR_INVALID (codes 1 .. 6) /
// LOC_ERR_UNSUPPORTED (code 7) and leaves the window as it was (densify: its table rows become diag(p_val[12..17]) all the same)
hipError_t launch_window_slide_dev(const SlideArgs& s, int n_anchors, int32_t* admit, bool densify, hipStream_t stream);

// the resident plain-drop slide of 6-DoF chain windows (window_slide_plain_kernel.hip; DESIGN.md §2, "The plain drop for 6-DoF chain
// windows"): one wave per window, in place on the resident batch's tables, one launch, nothing carried.  The host has admitted NOTHING: drop
// (may be nullptr: every window drops), new_pose and the new rows are the caller's device arrays; each wave admits its own window against
// slide_plain_admit.h's rule, writes admit[b] / status[b] (each may be nullptr: LOC_OK, LOC_ERR_INVALID for codes 1 .. 6 and 8,
// LOC_ERR_UNSUPPORTED for code 9) and either re-packs the window or leaves it as it was.
struct SlidePlainArgs {
    int32_t* counts; double* poses; double* poses_in;   // [B][4]; the optimised estimates x (read, then re-packed); the next solve's input estimates
    int32_t* r_idx; double* r_val; int32_t* p_idx; double* p_val; int32_t* s_idx; double* s_val;
    const int32_t* drop;                                 // [B] != 0: the window drops slot 0
    const double* new_pose;                              // [B][12]
    const int32_t* new_r_counts; const int32_t* new_r_idx; const double* new_r_val;   // [B], [B][nr_new_max][2], [B][nr_new_max][5]
    const int32_t* new_p_counts; const double* new_p_val;                             // [B], [B][np_new_max][18]
    const int32_t* new_s_counts; const int32_t* new_s_idx; const double* new_s_val;   // [B], [B][ns_new_max][4], [B][ns_new_max][48]
    int32_t* status; int32_t* admit;                                                  // [B], [B]
    int nr_new_max, np_new_max, ns_new_max;
    int n_anchors;    // the anchor table's size at call time: new anchor codes are admitted against it
    int pair_rule;    // SlidePairRule (slide_plain_admit.h): the pair rule of the resident verdict
    int B;
    WindowCaps caps;
};
hipError_t launch_window_slide_plain(const SlidePlainArgs& s, hipStream_t stream);

// the newest pose and the factors of every resident window from one raw message per window (window_message_kernel.hip; DESIGN.md §2, "Rows
// from raw messages"): one wave per window evaluates message_rows.h's rule at the window's count and newest solved pose and writes the
// arrays the two slides above read, at the capacities kMsgNrNew / kMsgNpNew / kMsgNsNew.  All device arrays; a message array may be nullptr
// when its bit is not in kinds_mask; verdict may be nullptr.
struct MessageArgs {
    const int32_t* counts; const double* poses;          // [B][4]; [B][nv_max][12] the optimised estimates
    const double* anchors; const double* antenna_xyz;    // [n_anchors][3]; [n_antenna][3]
    int n_anchors, n_antenna;
    int trajectory_length; double maximum_velocity, distance_outlier;
    int kinds_mask;
    const int32_t* kind; const double* dt;                                                                   // [B], [B]
    const int32_t* anchor; const int32_t* antenna; const float* distance; const float* distance_err;        // [B] each (RANGE)
    const double* imu; const double* lidar_z; const double* twist;                                           // [B][7], [B], [B][42]
    int32_t* drop_oldest; double* new_pose;                                                                  // [B], [B][12]
    int32_t* new_r_counts; int32_t* new_r_idx; double* new_r_val;                                            // [B], [B][2][2], [B][2][5]
    int32_t* new_p_counts; double* new_p_val;                                                                // [B], [B][2][18]
    int32_t* new_s_counts; int32_t* new_s_idx; double* new_s_val;                                            // [B], [B][1][4], [B][1][48]
    int32_t* verdict;                                                                                        // [B]
    int B, nv_max;
};
hipError_t launch_window_message_rows(const MessageArgs& a, hipStream_t stream);

// the per-edge chi2 audit and the outlier-range removal (edge_audit_kernel.hip; DESIGN.md §2, "Edge audit and outlier removal"): one wave per
// window at a.poses, every structure; a.r_off1 / a.p_info as the handle has them.  All device arrays.
struct EdgeAudit {
    double *r_chi2, *p_chi2, *s_chi2;   // the audit's outputs, [B][nr_max] / [B][np_max] / [B][ns_max] (slots beyond a window's count: 0), each may be nullptr
    double* total; int32_t* active;     // [B], each may be nullptr
    // the removal (prune_r_val != nullptr: a.r_val itself, writable; the audit's outputs are then not written): a window with active > min_edges
    // gets information 0.0 and removed = 1 on every range row with information != 0 and chi2 > chi2_max
    double* prune_r_val;
    double chi2_max; int min_edges;
    int32_t *removed, *n_removed;       // [B][nr_max], [B], each may be nullptr
};
hipError_t launch_window_edge_audit(const WindowArgs& a, const EdgeAudit& x, hipStream_t stream);

// the publish step and the path of a resident batch (window_publish_kernel.hip; DESIGN.md §2, "Publish and path records of a resident
// batch"): one lane per record, pose_records.h's rule at `poses`; reads counts, poses and result alone.  All device arrays; the host has
// checked 1 <= trajectory_length <= nv_max and 0 <= first, 1 <= count, first + count <= trajectory_length.
struct PublishArgs {
    const int32_t* counts; const double* poses; const double* result;   // [B][4]; [B][nv_max][12]; [B][8]
    double minimum_optimize_error; int trajectory_length;
    int32_t* flags;                      // [B]     bit 0: published, bit 1: the optimized pose is in the window
    double *realtime, *optimized;        // [B][7]  written only with bit 0 / bits 0 and 1; each may be nullptr
    double* chi2; int32_t* n_published;  // [B] always written; one count, zeroed on the stream by the launch; each may be nullptr
    long long B; int nv_max;
};
hipError_t launch_window_publish(const PublishArgs& a, hipStream_t stream);
struct PathArgs {
    const int32_t* counts; const double* poses;   // [B][4]; [B][nv_max][12]
    int trajectory_length, first, count;
    double* path; int32_t* present;               // [B][count][7] written only where present; [B][count]
    long long B; int nv_max;
};
hipError_t launch_window_path(const PathArgs& a, hipStream_t stream);

// the admission and the chain-family structure scan of a batch in the caller's DEVICE arrays (window_admit_kernel.hip; DESIGN.md §2, "Upload
// from device arrays"): one wave per window applies window_admit.h's rule and writes admit[b] (may be nullptr) and flags[b]; each wave leaves
// one partial record and a second launch of one wave merges them into *record.  All device arrays at the capacities `caps`; the host has
// checked NOTHING of their contents.  partial: kAdmitMaxWaves records.  s_val is not read and not passed.
struct WindowAdmitRecord;   // window_admit.h
constexpr int kAdmitMaxWaves = 8192;
struct WindowAdmitArgs {
    const int32_t* counts; const double* poses;
    const int32_t* r_idx; const double* r_val; const int32_t* p_idx; const double* p_val; const int32_t* s_idx;
    int32_t* admit; uint64_t* flags;                      // [B] window_admit's code; [B] window_structure_flags' word (0 for a refused window)
    WindowAdmitRecord* partial; WindowAdmitRecord* record;
    int n_anchors;
    long long B;
    WindowCaps caps;
};
int window_admit_waves(long long B);   // the waves launch_window_admit starts for B windows (= the partial records it writes)
hipError_t launch_window_admit(const WindowAdmitArgs& a, hipStream_t stream);

// the forest and arrowhead verdicts of an ADMITTED batch in device arrays, and arrow3_lm_kernel's tables (window_structure_kernel.hip; DESIGN.md
// §2, "Upload from device arrays"; option "upload_dev_structures"): arrow_pack.h's rule, one wave per window.  launch_window_structure writes
// hdr / rslot of every window (arrow != 0) and one partial record per wave, a one-wave launch merges them into *record; launch_window_arrow_pack
// writes rec / prec, the fill included, at the sizes the host took from that record.  All device arrays at the capacities `caps`.
struct WindowStructRecord;   // arrow_pack.h
constexpr int kStructMaxWaves = 2048;
struct WindowStructArgs {
    const int32_t* counts; const int32_t* r_idx; const int32_t* p_idx; const int32_t* s_idx;
    int32_t* hdr; int32_t* rslot;                         // [B][8], [B][nv_max]: ArrowAux's (arrow != 0)
    WindowStructRecord* partial; WindowStructRecord* record;   // kStructMaxWaves records; the batch's
    int arrow, forest;                                    // which of the two verdicts is wanted (the other bit of the record is 0)
    long long B;
    WindowCaps caps;
};
struct ArrowPackArgs {
    const int32_t* counts; const int32_t* r_idx; const double* r_val; const int32_t* p_idx; const double* p_val;
    const int32_t* hdr;                                   // [B][8] as launch_window_structure wrote it
    double* rec; double* prec;                            // [B][nchunk][jmax][64][3], [B][nchunk][jpmax][64][7]
    int jmax, jpmax, nchunk;
    long long B;
    WindowCaps caps;
};
size_t window_structure_lds_bytes(const WindowCaps& c);   // launch_window_structure's, arrow != 0 (four waves' row counters)
hipError_t launch_window_structure(const WindowStructArgs& a, hipStream_t stream);
hipError_t launch_window_arrow_pack(const ArrowPackArgs& a, hipStream_t stream);

// the grouping of an ADMITTED batch of forest windows of differing topologies in device arrays (window_groups_kernel.hip; DESIGN.md §2, "Upload
// from device arrays"; option "upload_dev_forest_groups"): passes 1 and 2 of build_tree_groups by window_groups.h's key, one wave per window.
// launch_window_groups zeroes the table on the stream and runs four launches — hash and insert; look up and verify, one partial record per
// wave; a one-wave merge into *record; a one-workgroup scan that numbers the groups by first appearance into sched_of / rep.
// launch_window_groups_gather copies the G representatives' counts and used index rows into the compact tables c_* at the capacities `caps`.
// All device arrays.  hash / rep0 / sched_of / rep: [B]; tab_key / tab_inv: `slots` entries (groups_table_slots(B), a power of two),
// contiguous — tab_inv directly behind tab_key — so that one memset clears both; partial: kGroupsMaxWaves records.
struct WindowGroupsRecord;   // window_groups.h
constexpr int kGroupsMaxWaves = 2048;
struct WindowGroupsArgs {
    const int32_t* counts; const int32_t* r_idx; const int32_t* p_idx; const int32_t* s_idx;
    uint64_t* hash;                                       // [B] the masked hash of window b's key (0: the window was not hashed)
    uint64_t* tab_key; uint32_t* tab_inv;                 // open-addressed: a slot's hash (0: empty) and ~(the lowest window index that carries it)
    uint64_t slots;
    int32_t* rep0; int32_t* sched_of; int32_t* rep;       // [B] the lowest window of b's hash; b's group; group g's first window
    WindowGroupsRecord* partial; WindowGroupsRecord* record;
    int hash_bits;                                        // option "upload_dev_groups_hash_bits"
    long long B;
    WindowCaps caps;
};
struct WindowGroupsGatherArgs {
    const int32_t* counts; const int32_t* r_idx; const int32_t* p_idx; const int32_t* s_idx;
    const int32_t* rep;                                   // [G]
    int32_t* c_counts; int32_t* c_r_idx; int32_t* c_p_idx; int32_t* c_s_idx;   // [G][4], [G][nr_max][2], [G][np_max], [G][ns_max][4]
    long long G, B;
    WindowCaps caps;
};
hipError_t launch_window_groups(const WindowGroupsArgs& a, hipStream_t stream);
hipError_t launch_window_groups_gather(const WindowGroupsGatherArgs& a, hipStream_t stream);

size_t window_tree_workspace_doubles(const WindowCaps& c, long long B);
hipError_t launch_window_tree(const WindowArgs& a, const TreeSched& ts, double* ws, hipStream_t stream);
hipError_t launch_window_tree_wave(const WindowArgs& a, const TreeSched& ts, hipStream_t stream);
// the per-window-schedule twin (tree_wave_kernel.hip: tree_wave_groups_kernel).  host_hdr: the host's copy of g.hdr — every group's sizes are
// held to launch_window_tree_wave's bounds (and one EdgeSE3 per node) BEFORE the launch; hipErrorInvalidValue otherwise, and for B <= 0
hipError_t launch_window_tree_wave_groups(const WindowArgs& a, const TreeGroups& g, const int32_t* host_hdr, hipStream_t stream);

}  // namespace locamd
