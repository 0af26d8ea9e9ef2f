/*
 * localization_amd — C ABI of the MI355X-native range-localization solver.
 *
 * The reference (sair-lab/localization) has no plugin/FFI seam: class Localization owns a
 * g2o::SparseOptimizer by value (reference src/localization/localization.h:168) and calls it directly.
 * The boundary cut here is exactly the set of g2o calls Localization/Robot make; every
 * entry point below names the reference call site(s) it replaces.  Plain pointers and sizes only; no
 * exceptions cross the ABI; every function returns a loc_status (0 = OK, <0 = error).
 *
 * There is NO CPU fallback: creating a solver without a usable HIP device fails with LOC_ERR_NO_DEVICE.
 *
 * Threading: like the reference (one ros::spin() thread, localization_node.cpp:98) a handle is not
 * thread-safe; distinct handles are independent.  All device work of a handle is issued on the HIP stream
 * the caller passes (or the handle's own stream when NULL).
 */
#ifndef LOCALIZATION_AMD_H
#define LOCALIZATION_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LOC_ABI_VERSION 4 /* 2: jacobian mode for every solver, resident window solves, loc_node_add_rl_range;
                           * 3: numeric (g2o) Jacobians are the default everywhere, loc_shard_*, loc_window_last_kernel_kind;
                           * 4: loc_window_set_option / _last_host_timing, loc_node_flush_tail / _last_kernel_kind, loc_fusion_timing_*;
                           *    a large loc_window_solve_host drops the resident batch;
                           *    (additive, same version) loc_window_covariance_host / _resident / loc_window_last_covariance_ms / loc_window_covariance_plan;
                           *    (additive, same version) loc_window_joint_covariance_host / _resident / _plan;
                           *    (additive, same version) loc_snapshot_solve_device_cov / _host_kmb_cov, loc_fusion_solve_device_cov / _host_kmb_cov */

typedef enum loc_status {
    LOC_OK = 0,
    LOC_ERR_INVALID = -1,      /* bad argument / shape */
    LOC_ERR_NO_DEVICE = -2,    /* no HIP device: the product path refuses to run */
    LOC_ERR_HIP = -3,          /* a HIP runtime call failed (see loc_last_error) */
    LOC_ERR_UNKNOWN_NODE = -4, /* node id not in nodesId (reference: std::map::at throws, localization.cpp:306) */
    LOC_ERR_UNSUPPORTED = -5,  /* shape outside what the kernels are built for */
    LOC_ERR_SINGULAR = -6      /* non-invertible covariance (reference: MatrixXd::inverse, localization.cpp:277,601) */
} loc_status;

/* Range-edge Jacobian. The reference inherits g2o's numeric central difference (delta = 1e-9) because
 * EdgeSE3Range does not override linearizeOplus (types_edge_se3range.h:45-74).  ANALYTIC is the exact
 * derivative of the same residual (0 where the endpoints coincide, which is what the numeric form gives). */
enum { LOC_JAC_ANALYTIC = 0, LOC_JAC_NUMERIC_G2O = 1 };

const char* loc_last_error(void);  /* thread-local message of the last failing call */
int32_t loc_abi_version(void);
int32_t loc_device_count(void);    /* 0 when no HIP device is visible */

/* ================================================================================================
 * Multi-GPU shard descriptor (SURVEY.md §8(b) "device selection + stream; multi-GPU shard descriptor", §8(e)).
 * Tags / windows / hypotheses are independent least-squares problems (one Localization object each in the reference:
 * localization_node.cpp:46), so a batch of `total` instances is split into contiguous slices of ceil(total / world)
 * instances, one per rank = one process = one GPU; anchors and parameters are replicated; there is NO collective on
 * the solve path.  Host-only helpers (no device needed): a C++ caller computes its slice with the same rule the Python
 * harness and bench.py use.
 * ============================================================================================== */
typedef struct loc_shard {
    int32_t rank, world;   /* this slice belongs to rank `rank` of `world` */
    int32_t device;        /* HIP device index on the rank's node: rank % devices_per_node */
    int32_t reserved;
    int64_t lo, hi;        /* instances [lo, hi) of the batch; hi - lo may be 0 for trailing ranks */
} loc_shard;
/* [lo, hi) of rank `rank`; LOC_ERR_INVALID unless total >= 0 and 0 <= rank < world */
int loc_shard_bounds(int64_t total, int32_t rank, int32_t world, int64_t* lo, int64_t* hi);
/* fills out[0 .. world-1]; devices_per_node <= 0: loc_device_count() (LOC_ERR_NO_DEVICE when that is 0) */
int loc_shard_plan(int64_t total, int32_t world, int32_t devices_per_node, loc_shard* out);

/* ================================================================================================
 * Batched snapshot solver — BASELINE config 2 (8-anchor UWB, B independent tags, 3-DoF position).
 *
 * One "update" = for one tag, ingest one epoch of M anchor ranges and run what the reference runs per
 * solve: create_range_edge per range (information 1/err^2, RobustKernelCauchy delta 1;
 * localization.cpp:608-627, :318), the outlier gate on the prior estimate (:306-313), then
 * Localization::solve() = initializeOptimization + optimize(maximum_iteration) with g2o's
 * Levenberg-Marquardt (:164-170), then optimizer.chi2() (:197).  With identity antenna offsets the
 * 6-DoF g2o problem reduces exactly to a 3x3 one (SURVEY.md §8(a) note), which is what the kernel solves.
 *
 * Device layouts (all device pointers unless the name says host):
 *   dist, err : float  [K][M4][B][4]   M4 = ceil(M/4); anchor m sits at [m/4][..][m%4]; padded lanes err = 0
 *   pos       : double [3][B]          state carried across epochs (in: prior/initial estimate, out: last)
 *   out_pos   : double [K][3][B]       estimate after each epoch's solve
 *   out_chi2  : double [K][B]          optimizer.chi2() after each solve (non-robust, last evaluated state)
 *   out_trials: uint8  [K][B] or NULL  number of LM trials (linear solves) spent
 * ============================================================================================== */
typedef struct loc_snapshot loc_snapshot;

typedef struct loc_snapshot_params {
    int32_t maximum_iteration;   /* optimizer/maximum_iteration, localization.cpp:65 (default 20; cfg yaml: 10) */
    double distance_outlier;     /* robot/distance_outlier, localization.cpp:78; <= 0 disables the gate */
    int32_t gate_warmup_epochs;  /* epochs after (re)initialisation that run un-gated: the reference gates only once
                                    number_measurements > trajectory_length (localization.cpp:309). default 1 */
    int32_t jacobian;            /* LOC_JAC_*; loc_snapshot_default_params: LOC_JAC_NUMERIC_G2O (the reference's configuration) */
    int32_t lanes_per_instance;  /* 0 = library default; otherwise 1,2,4,8 (must divide the padded anchor count) */
    int32_t block_threads;       /* 0 = default (256) */
} loc_snapshot_params;

void loc_snapshot_default_params(loc_snapshot_params* p);

/* anchors_xyz_host: [M][3] doubles = /uwb/nodesPos of the static nodes (localization.cpp:86-108). */
int loc_snapshot_create(loc_snapshot** out, int32_t device, int64_t batch, int32_t n_anchors,
                        const double* anchors_xyz_host, const loc_snapshot_params* params);
int loc_snapshot_destroy(loc_snapshot* s);

int64_t loc_snapshot_batch(const loc_snapshot* s);
int32_t loc_snapshot_anchor_groups(const loc_snapshot* s);         /* M4 */
int32_t loc_snapshot_lanes_per_instance(const loc_snapshot* s);
/* number of floats in a dist/err buffer for `epochs` epochs = epochs * M4 * B * 4 */
size_t loc_snapshot_range_floats(const loc_snapshot* s, int32_t epochs);

/* Robot::init estimate (robot.cpp:47) for every tag: host [3][B] doubles -> device state, and back.
 * Setting positions restarts the gate warm-up (epoch counter = 0). */
int loc_snapshot_set_positions(loc_snapshot* s, const double* pos_soa_host);
int loc_snapshot_get_positions(loc_snapshot* s, double* pos_soa_host);
void* loc_snapshot_positions_device(loc_snapshot* s); /* the [3][B] device state itself */
int64_t loc_snapshot_epochs_done(const loc_snapshot* s);
int loc_snapshot_set_epochs_done(loc_snapshot* s, int64_t epochs);

/* Pack host ranges given as [K][M][B] (anchor-major SoA) into the device tile layout [K][M4][B][4]. */
int loc_snapshot_pack_ranges_host(const loc_snapshot* s, int32_t epochs, const float* src_kmb, float* dst_tiles,
                                  float pad_value);

/* The hot path: K epochs for all B tags, inputs and outputs resident in HBM. Asynchronous on hip_stream. */
int loc_snapshot_solve_device(loc_snapshot* s, int32_t epochs, const float* dist_dev, const float* err_dev,
                              double* out_pos_dev, double* out_chi2_dev, uint8_t* out_trials_dev,
                              void* hip_stream);

/* Convenience: same, with host buffers in the tile layout (stages over PCIe, synchronous). */
int loc_snapshot_solve_host(loc_snapshot* s, int32_t epochs, const float* dist_tiles_host,
                            const float* err_tiles_host, double* out_pos_host, double* out_chi2_host,
                            uint8_t* out_trials_host);

/* The batched mirror of the reference's per-message callback for callers that hold plain host arrays
 * (SURVEY.md 8(b) `batch_push_ranges` + `batch_solve` + `batch_get_positions`): distance / distance_err as
 * [K][M][B] float32 (epoch, anchor, tag — what K rounds of addRangeEdge, localization.cpp:297-376, would have been fed),
 * outputs [K][3][B] / [K][B].  Copy-in, tile packing + solve, and copy-out run as a chunked three-stream pipeline, so the
 * call costs about max(PCIe in, solve, PCIe out) rather than their sum — when the host buffers are page-locked
 * (loc_host_alloc); with pageable memory the result is the same, the copies just do not overlap.  Synchronous. */
int loc_snapshot_solve_host_kmb(loc_snapshot* s, int32_t epochs, const float* dist_kmb_host, const float* err_kmb_host,
                                double* out_pos_host, double* out_chi2_host, uint8_t* out_trials_host);

/* Per-update marginal covariances: the same solve, bit for bit (positions, chi2, trials), plus for every tag and epoch
 * Sigma = H^-1 with H = sum_m J_m^T (rho'_m Omega_m) J_m the undamped system of the update AT the emitted position: rho'_m = 1 / (1 + chi2_m)
 * (Cauchy), J_m in the handle's Jacobian mode, over the update's active ranges only — "the gate's weights": a range the outlier gate
 * rejected on the prior (or an invalid slot) is not in H.  H is the one the LM loop already holds, so nothing is relinearised.
 *   cov    double [K][6][B]  xx xy xz yy yz zz; NaN when singular
 *   mask   int32  [K][B]     bits 0-2 = tx ty tz: a coordinate whose diagonal entry of H is exactly 0 is excluded (its entries are 0)
 *   status int32  [K][B]     LOC_OK, or LOC_ERR_SINGULAR: a pivot of H's LDL^T is not finite, not positive or at most 1e-11 of its
 *                            diagonal entry
 * A tag without an active range gets every mask bit, zeros and LOC_OK.  LOC_ERR_INVALID (nothing launched) if a handle or any of the three
 * covariance pointers is NULL; the other arguments as loc_snapshot_solve_device / _host_kmb (host arrays for the _host_kmb form). */
int loc_snapshot_solve_device_cov(loc_snapshot* s, int32_t epochs, const float* dist_dev, const float* err_dev,
                                  double* out_pos_dev, double* out_chi2_dev, uint8_t* out_trials_dev,
                                  double* out_cov_dev, int32_t* out_cov_mask_dev, int32_t* out_cov_status_dev, void* hip_stream);
int loc_snapshot_solve_host_kmb_cov(loc_snapshot* s, int32_t epochs, const float* dist_kmb_host, const float* err_kmb_host,
                                    double* out_pos_host, double* out_chi2_host, uint8_t* out_trials_host,
                                    double* out_cov_host, int32_t* out_cov_mask_host, int32_t* out_cov_status_host);

/* Page-locked host memory for the host paths above (hipHostMalloc / hipHostFree). */
int loc_host_alloc(void** out, size_t bytes);
int loc_host_free(void* p);

/* HIP-event timing of the solve kernel on the stream it is launched on (bench.py's roofline leg).
 * loc_snapshot_timing_begin() arms per-launch event pairs; _end() synchronises and returns the number of
 * timed launches, their total and average duration in milliseconds. */
int loc_snapshot_timing_begin(loc_snapshot* s, int32_t max_launches);
int loc_snapshot_timing_end(loc_snapshot* s, int32_t* n_launches, double* total_ms, double* avg_ms);


/* ================================================================================================
 * Batched sliding-window graph solver — the reference's general case (BASELINE configs 1, 3, 5 shapes):
 * B independent instances, each the graph one Localization object holds when it calls solve()
 * (localization.cpp:164-170): moving VertexSE3 poses (robot.cpp:75-110), fixed anchors, EdgeSE3Range factors
 * with an antenna lever arm on endpoint 0 (localization.cpp:331-340, types_edge_se3range.cpp:105-114; endpoint 1's through
 * loc_window_set_endpoint1_offsets),
 * EdgeSE3Prior with diagonal information (IMU / lidar, localization.cpp:476-486, 513-525) and EdgeSE3
 * (pose / twist, localization.cpp:263-281, 588-602).  Range and SE3 edges carry RobustKernelCauchy(1) as in the
 * reference (range always; SE3 per the `robust` flag); priors do not.  Range Jacobians: g2o's central differences by default
 * (the reference's configuration, types_edge_se3range.h:45-74); analytic ones with loc_window_set_jacobian.
 *
 * Host layouts (arrays of B instances, fixed capacities per instance):
 *   counts int32 [B][4]           nv, nr, np, ns  (poses, range edges, priors, SE3 edges actually used)
 *   poses  double[B][nv_max][12]  R row-major (9), t (3); in: estimates, out: optimised estimates
 *   r_idx  int32 [B][nr_max][2]   v0 = pose slot; v1 = pose slot, or -1 - anchor_index for a fixed anchor
 *   r_val  double[B][nr_max][5]   measurement, information (1/cov), lever arm xyz of endpoint 0
 *   p_idx  int32 [B][np_max]      pose slot
 *   p_val  double[B][np_max][18]  INVERSE measurement Z^-1 as R(9), t(3); information diagonal (6)
 *   s_idx  int32 [B][ns_max][4]   vi, vj, robust (0/1), 0
 *   s_val  double[B][ns_max][48]  INVERSE measurement Z^-1 as R(9), t(3); information 6x6 row-major
 *   result double[B][8]           chi2() over all edges at the last evaluated state, robust chi2 of the accepted
 *                                 state, final lambda, outer iterations run, LM trials, terminated flag, [6] number of
 *                                 pose-to-pose edges that share their pair of poses with another edge, [7] diagnostics of
 *                                 the factorisation (windows of <= 512 poses): elimination levels * 65536 + blocks of the
 *                                 factor + (poses in the dense root supernode) / 16; the one-lane-per-window kernel
 *                                 reports nv * 65536 + 2 nv - 1
 * The normal equations are kept as sparse 6x6 blocks (storage sized from the envelope bound nv_max * bw_max: per pose,
 * columns from its leftmost neighbour to itself), so storage and work scale with nv_max * bw_max^2, not nv_max^3:
 * cfg/uwb_pose.yaml's 500-pose chain is 3000 rows of ~12 entries.
 * Windows whose per-instance arrays fit 160 KiB keep everything in LDS (loc_window_lds_bytes tells); larger ones keep
 * them in a per-instance slice of an HBM workspace the handle allocates (a few MB for 500 poses).
 * ============================================================================================== */
typedef struct loc_window loc_window;
typedef struct loc_window_caps {
    int32_t nv_max, nr_max, np_max, ns_max;
    int32_t bw_max; /* widest pose-to-pose coupling |vi - vj| of any binary edge, in pose slots; < 0 = nv_max - 1 (dense).
                     * Pass the true bound: it sizes the per-instance storage, and small windows then fit twice as many
                     * instances per CU (measured: 4096 ten-pose chains 3.3 ms with -1, 1.8 ms with 1). */
} loc_window_caps;

int loc_window_create(loc_window** out, int32_t device, int64_t batch, const loc_window_caps* caps,
                      int32_t n_anchors, const double* anchors_xyz_host, int32_t maximum_iteration);
int loc_window_destroy(loc_window* w);
/* replace the fixed-vertex table (re-uploads; grows the device buffer when needed) */
int loc_window_set_anchors(loc_window* w, int32_t n_anchors, const double* anchors_xyz_host);
size_t loc_window_lds_bytes(const loc_window_caps* caps);
/* Synchronous: stages the B instances over PCIe, runs one launch, copies poses and results back. */
int loc_window_solve_host(loc_window* w, int64_t n_instances, const int32_t* counts, double* poses,
                          const int32_t* r_idx, const double* r_val, const int32_t* p_idx, const double* p_val,
                          const int32_t* s_idx, const double* s_val, double* result);
/* kernel time of the last loc_window_solve_host launch (HIP events on its stream), milliseconds */
int loc_window_last_kernel_ms(loc_window* w, double* ms);
/* EdgeSE3Range carries a lever arm per ENDPOINT (Isometry3d offset[2], types_edge_se3range.h:73; setVertexOffset(int, ...),
 * types_edge_se3range.cpp:99-103; both used in the residual, :108-112).  r_val holds endpoint 0's — the only one the reference
 * ever sets (localization.cpp:334).  This call supplies endpoint 1's for the instances of every LATER solve / upload: off1 =
 * [n_instances][nr_max][3] (xyz per range edge; for a fixed endpoint 1 — identity rotation — the point is the anchor + o1), or
 * NULL to go back to none.  Batches with endpoint-1 lever arms are solved by the general kernel (LOC_WINDOW_KERNEL_GENERAL). */
int loc_window_set_endpoint1_offsets(loc_window* w, int64_t n_instances, const double* off1_xyz);
/* g2o's EdgeSE3Prior takes a full 6x6 information matrix (a pose source with a full covariance, the marginal prior of a dropped pose:
 * loc_window_marginal_prior_host); p_val holds a diagonal.  This call supplies full matrices for the EdgeSE3Prior factors of every LATER
 * solve / upload / covariance / marginal-prior call: pinfo = [n_instances][np_max][36], row-major, order (tx ty tz qx qy qz) as s_val's; row e
 * REPLACES the diagonal p_val[b][e][12..17] (which is then not read).  NULL: back to the diagonals.  Everything is checked before anything
 * changes: LOC_ERR_INVALID for n_instances <= 0 or beyond the handle's batch, for a solver without priors (np_max = 0) and for a matrix
 * that is not exactly symmetric (W[i][j] != W[j][i]; every row of the n_instances * np_max is looked at, unused ones included).  While a
 * table of n instances is set, a call with more than n instances is LOC_ERR_INVALID.  Priors stay non-robust: chi2 = e^T W e,
 * H += J^T W J, b -= J^T W e.  Such a handle solves on the general kernel (LOC_WINDOW_KERNEL_GENERAL), and its covariances come from the
 * envelope pass alone (option "covariance_general" = 1; LOC_ERR_UNSUPPORTED with nothing written otherwise) — unless option
 * "prior_information_structured" is 1 and the table is translation-only (see loc_window_set_option).  The device table is
 * allocated by the first call and freed with the handle. */
int loc_window_set_prior_information(loc_window* w, int64_t n_instances, const double* pinfo);
/* LOC_JAC_NUMERIC_G2O (default: the reference's configuration) or LOC_JAC_ANALYTIC (opt-in fast mode) for the EdgeSE3Range
 * factors of every later solve */
int loc_window_set_jacobian(loc_window* w, int32_t jacobian);
/* Windows of up to 512 poses are eliminated in a minimum-degree order the kernel computes per instance (what CHOLMOD's AMD
 * ordering does for the reference, localization.h:82-84: a key-frame star then factors without fill, a chain with a dense
 * border is dissected into ~log2(n) levels); natural != 0 keeps the caller's pose order instead, and so does a window
 * whose fill under that order would not fit the storage bw_max sized.  Larger windows (513 ... 1024 poses) always use the
 * caller's order (loc_node_* packs them leaf-first). */
int loc_window_set_ordering(loc_window* w, int32_t natural);
/* Large batches of CHAIN windows — every pose-to-pose edge (range or SE3) joins consecutive poses (the smoothness edge of
 * Robot::new_vertex, robot.cpp:75-110; addTwistEdge's EdgeSE3, localization.cpp:438-459), edges listed in the order of their later
 * pose and priors in pose order (the order addRangeEdge / addImuEdge / addTwistEdge create them in: cfg/uwb_only.yaml,
 * cfg/uwb_imu.yaml, cfg/uwb_imu_lidar.yaml, cfg/uwb_twist.yaml) — are solved one GPU lane per window by a block-tridiagonal
 * kernel (same LM, elimination in pose order).  min_batch: the smallest batch that takes that
 * path (default 12 288, or LOCAMD_CHAIN_MIN_BATCH from the environment; 0: never; < 0: back to the default). */
int loc_window_set_chain_threshold(loc_window* w, int64_t min_batch);
/* Which kernel the last solve of this handle ran (the choice depends on the batch: its size and structure).
 *   GENERAL  window_lm_kernel: one wave (65 ... 512 poses: eight waves) per window, sparse block Cholesky in a minimum-degree order
 *   CHAIN    chain_lm_kernel: one lane per window, block-tridiagonal 6x6 (batches >= the chain threshold of chain windows)
 *   CHAIN3   chain3_lm_kernel: the same for TRANSLATION-ONLY batches (windows of more than 64 poses from 4 096 windows on; windows of <= 64
 *            poses only past an explicit threshold: WAVE3 serves those at every batch size) — no EdgeSE3, every lever arm zero, every rotation the
 *            identity (what Robot::init, robot.cpp:47, and the default identity antenna offsets, localization.h:170, give:
 *            cfg/uwb_only.yaml on the example bag), priors without rotation information: the 6-DoF problem then reduces EXACTLY
 *            to 3x3 blocks (types_edge_se3range.cpp:105-114 does not see the rotation; SURVEY.md §8(a) note)
 *   ARROW3   arrow3_lm_kernel: one wave per window for TRANSLATION-ONLY windows that are a chain with a small dense border — a
 *            trajectory whose poses range to up to 12 nodes that are unknowns themselves, held in the LAST pose slots (anchor
 *            self-calibration, BASELINE config 4; "every node moves", localization.cpp:94-98): the chain cut into four segments
 *            (one wave each), block-tridiagonal sweeps + the border's Schur complement on the f64 matrix cores; taken by
 *            windows of more than 64 poses (any batch size)
 *   TREE     tree_wave_kernel: batches (>= 256 windows) in which EVERY window has the same structure (same counts and index
 *            tables: one graph replayed with different measurements) and that structure is a forest of up to 64 poses (BASELINE
 *            config 5: the key-frame star of addPoseEdge, localization.cpp:254-290, + one anchor range per pose).  The fill-free
 *            elimination schedule is computed once on the host; one wave per window with LANE = POSE and a pose's whole solver
 *            state in that lane's registers (no workspace in memory), elimination by height.  (Nodes with several EdgeSE3 to
 *            their parent: tree_lm_kernel, one lane per window on the same schedule.)
 *   WAVE3   a translation-only chain batch (as CHAIN3) of windows of <= 64 poses, any batch size — in particular the drop-in node's
 *            own solve, one window per range message: wave3_lm_kernel, one wave per window, lane = edge for the residuals /
 *            Jacobians, lane = pose for the 3x3-block normal equations, rank-1 couplings solved by a scalar recurrence handed from
 *            lane to lane, the next LM trials' lambdas solved speculatively in the idle lanes.
 *   WAVE6   the 6-DoF sibling of WAVE3 (IMU / lidar priors, an antenna lever arm on the pose): chain windows of <= 64 poses without
 *            EdgeSE3 factors and with at most one range edge per pair of consecutive poses, any batch size (an explicit chain threshold
 *            hands larger batches to CHAIN).
 *   WAVE6S  the same kernel with FULL coupling blocks (wave6_lm_kernel<JAC, SE3>): chain windows of <= 63 poses WITH an EdgeSE3 factor between
 *            consecutive poses — Localization::addTwistEdge (localization.cpp:438-459, cfg/uwb_twist.yaml) — at most one per pair, at
 *            most one range edge per pair; the block Cholesky runs from both ends of the chain towards the middle pose.  Switched by
 *            option "wave6" as well.
 * All of them run the same LM and agree to the tolerances of DESIGN.md §3; result[6] / result[7] keep their meaning (the
 * lane-per-window kernels eliminate in pose order: result[7] = nv * 65536 + 2 nv - 1). */
enum { LOC_WINDOW_KERNEL_NONE = -1, LOC_WINDOW_KERNEL_GENERAL = 0, LOC_WINDOW_KERNEL_CHAIN = 1, LOC_WINDOW_KERNEL_CHAIN3 = 2, LOC_WINDOW_KERNEL_ARROW3 = 3, LOC_WINDOW_KERNEL_TREE = 4,
       LOC_WINDOW_KERNEL_TREE_LANE = 5 /* reported only: the lane-per-window variant of TREE ran */,
       LOC_WINDOW_KERNEL_WAVE3 = 6 /* translation-only chains of <= 64 poses: one wave per window (wave3_lm_kernel) */,
       LOC_WINDOW_KERNEL_WAVE6 = 7 /* 6-DoF chains of <= 64 poses (no EdgeSE3, one range edge per consecutive pair): wave6_lm_kernel */,
       LOC_WINDOW_KERNEL_WAVE6S = 8 /* the same with EdgeSE3 factors between consecutive poses (cfg/uwb_twist.yaml), at most one per pair: wave6_lm_kernel<.., SE3> */,
       LOC_WINDOW_KERNEL_TREE_GROUPS = 9 /* option "forest_groups": forest windows of DIFFERING topologies, one wave per window on the schedule of the
                                            window's group (tree_wave_kernel<JAC, TreeGroups>); TREE's batch threshold */ };
int loc_window_last_kernel_kind(const loc_window* w, int32_t* kind);
/* Kernel-selection switches of ONE handle.  They are read from the environment ONCE, when the handle is created (LOCAMD_CHAIN_MIN_BATCH,
 * LOCAMD_ARROW3, LOCAMD_TREE, LOCAMD_WAVE3, LOCAMD_WAVE6, LOCAMD_CHAIN3, LOCAMD_NO_ZERO_COPY: A/B runs and tests), never at solve
 * time; this call changes them afterwards.  name / value:
 *   "chain_min_batch"  as loc_window_set_chain_threshold (0: never anything but the general kernel; < 0: the default rule)
 *   "arrow3"           -1 default (windows of more than 64 poses), 0 never, 1 whenever the batch qualifies
 *   "tree"             -1 default, 0 never, 2 the lane-per-window variant (tree_lm_kernel)
 *   "wave3" "wave6" "chain3" "zero_copy"   1 (default) / 0
 *   "topology_cache"   1 (default) / 0: reuse the structural verdict of the previous batch when counts and index tables hash the same
 *   "kernel_events"    1 (default; LOCAMD_KERNEL_EVENTS) / 0: no HIP events around the launch of a zero-copy solve (a handful of small windows);
 *                      loc_window_last_kernel_ms then reports launch-to-completion on the host clock.  The node's own handle runs with 0.
 *   "covariance_general"  0 (default) / 1: loc_window_covariance_* also serve the batches their three structured passes decline (see there);
 *                      looked at per call; a resident batch classified under one value is classified again after a change
 *   "prior_information_structured"  0 (default) / 1: a handle whose table of full information matrices (loc_window_set_prior_information) is
 *                      TRANSLATION-ONLY — every matrix a dense 3x3 block on the translation, rotation rows and columns exactly 0: the rows
 *                      loc_window_marginal_prior_host returns — keeps the wave-per-window 3x3 kernels for translation-only CHAIN batches of
 *                      <= 64 poses: the solve runs on LOC_WINDOW_KERNEL_WAVE3 wherever a handle without a table would take it (options
 *                      "wave3" / "chain3", the chain threshold, the ordering override), and loc_window_covariance_* take the chain 3x3 pass
 *                      without "covariance_general".  While such a table is set p_val[12..17] is not read, by the structure test either.
 *                      Everything else on the handle — a table with a rotation entry, endpoint-1 lever arms, a batch that is no
 *                      translation-only chain, a batch the rules hand to another kernel — goes to the general kernel and the envelope pass
 *                      as with 0.  0: every call does what it did without the option, bit for bit.  Looked at per call; a resident batch whose
 *                      verdict was taken under a structured table solves on the general kernel once the table has gone, has got a rotation
 *                      entry or the option is 0 (until the next upload), and its covariance pass is classified again.
 *   "resident_slide"  0 (default) / 1: loc_window_upload keeps a host mirror of the batch's integer tables (counts, r_idx, p_idx), which
 *                      loc_window_slide_resident needs; read at upload time.  0: an upload allocates and does exactly what it did without the option.
 *   "forest_groups"   0 (default) / 1: a batch of FOREST windows of <= 64 poses whose topologies differ — key-frame windows cut from different
 *                      robots or at different phases of the key cadence (Localization::addPoseEdge, localization.cpp:254-290): other parents,
 *                      other lengths, other anchors — is grouped by topology (the four counts and the used index rows; anchor numbers and
 *                      robust flags do not count) and solved on LOC_WINDOW_KERNEL_TREE_GROUPS with one schedule per group, by
 *                      loc_window_solve_host and by loc_window_upload + loc_window_solve_resident.  Looked at only after the one-topology test
 *                      has declined the batch: a batch of one topology takes LOC_WINDOW_KERNEL_TREE as without the option, bit for bit.  The
 *                      batch stays on the general kernel when any window has fewer than 2 poses, a cycle, or two EdgeSE3 factors on one pair of
 *                      poses; under option "tree" = 0 or 2; below TREE's batch threshold; with endpoint-1 lever arms or a table of full
 *                      information matrices; on a handle with nv_max > 64.  loc_window_upload_dev groups only under option "upload_dev_forest_groups" (else such a
 *                      batch solves on the general kernel), and covariances of such a batch are served as without the option (the envelope pass under
 *                      "covariance_general", else LOC_ERR_UNSUPPORTED) unless option "forest_groups_covariance" is 1 as well.  Measured at 16 384 x 64 poses: the solve 3.5 ... 4.8 times faster than on
 *                      the general kernel for 1 ... 16 384 groups; the upload 3 ... 7 ms slower up to 256 groups and 46 ms slower (102 MB of
 *                      schedule tables) with a topology per window — there the option pays from the fourth resident solve on (README).
 *   "forest_groups_covariance"  0 (default) / 1: with "forest_groups" = 1, loc_window_covariance_* and loc_window_joint_covariance_* serve a
 *                      batch of forest windows of differing topologies on the forest pass, one wave per window on the schedule of the window's
 *                      group (see there).  0, or "forest_groups" = 0: every call takes the pass it took without the option, bit for bit.  Looked
 *                      at per call; a resident batch that was refused, or held by the envelope pass, is classified again after a change.
 *   "upload_dev_structures"  0 (default) / 1: loc_window_upload_dev also takes the ARROWHEAD and FOREST verdicts on the device (see there), so
 *                      that such a batch runs on LOC_WINDOW_KERNEL_ARROW3 / _TREE and their covariance passes exactly as after loc_window_upload
 *                      of the same arrays; read at upload time.  0: loc_window_upload_dev does exactly what it did without the option.
 *   "upload_dev_forest_groups"  0 (default) / 1: with "upload_dev_structures" = 1 and "forest_groups" = 1, loc_window_upload_dev groups a batch
 *                      of forest windows of differing topologies on the device (see there) and leaves the handle as loc_window_upload of the
 *                      same arrays does: LOC_WINDOW_KERNEL_TREE_GROUPS, the same groups block byte for byte, the same loc_window_forest_groups,
 *                      and under "forest_groups_covariance" the grouped covariance pass on the uploaded block from the first call on.  Read at
 *                      upload time.  0, or either of the other two options 0: loc_window_upload_dev does exactly what it did without the option.
 *   "upload_dev_groups_hash_bits"  0 ... 64 (default 64).  A TEST SEAM, not a tuning knob: the candidate hash of the device grouping pass is
 *                      masked to this many low bits before it is used, which forces hash collisions (0: every window collides with window 0).
 *                      The groups are defined by key equality and first appearance, so no value changes any answer; a collision only makes
 *                      the call group the batch on the host instead.
 * LOC_ERR_INVALID for an unknown name or value. */
int loc_window_set_option(loc_window* w, const char* name, int64_t value);
/* Host-side cost of the last loc_window_solve_host call, milliseconds: [0] argument validation, [1] structure analysis (kernel
 * choice: hash of the index tables, chain / forest / arrowhead tests, host-built schedules), [2] staging + launch + copy back +
 * synchronise, [3] 1.0 when the structural verdict came from the handle's cache, else 0.0 */
int loc_window_last_host_timing(const loc_window* w, double* validate_topology_run_cached);
/* Option "forest_groups": what the handle's LAST structural verdict — of a loc_window_solve_host call or of an upload (loc_window_upload, or
 * loc_window_upload_dev under option "upload_dev_forest_groups"), whichever came last —
 * found: the number of topology groups and the size in bytes of the block sent to the device (headers, window -> group map, the groups'
 * schedule tables).  0 and 0 when that batch is not on the grouped path. */
int loc_window_forest_groups(const loc_window* w, int32_t* n_groups, int64_t* table_bytes);
/* Device-resident operation: upload n instances once (same host layouts as loc_window_solve_host), then run
 * loc_window_solve_resident any number of times — each launch starts from the uploaded estimates, is asynchronous on
 * hip_stream (NULL = the handle's own stream) and leaves poses / result on the device — and fetch them with
 * loc_window_download (synchronises).
 * Mixing with loc_window_solve_host on the same handle: every loc_window_solve_host first waits for the last resident launch (a
 * handle-owned event; the caller's stream is not kept).  A SMALL host solve (its inputs fit the 4 MiB staging block) leaves the
 * resident batch intact.  A LARGE one reuses the resident batch's device arrays: it DROPS the resident batch — the next
 * loc_window_solve_resident / loc_window_download return LOC_ERR_INVALID until loc_window_upload is called again.  loc_window_timing_begin/_end bracket resident launches with HIP events on the
 * stream they run on, like loc_snapshot_timing_*. */
int loc_window_upload(loc_window* w, int64_t n_instances, const int32_t* counts, const double* poses,
                      const int32_t* r_idx, const double* r_val, const int32_t* p_idx, const double* p_val,
                      const int32_t* s_idx, const double* s_val);
/* loc_window_upload from DEVICE arrays ("Upload from device arrays"): the layouts are loc_window_upload's, every array is a device
 * array at the handle's capacities, alive and unchanged until the call returns, and none aliases the handle's own arrays (loc_window_poses_device
 * ...).  Nothing of the batch passes through host memory: one HIP pass on hip_stream (NULL = the handle's own) admits every window — the shape
 * check loc_window_upload runs on CPU threads, the same checks in the same order — and scans the structure of the chain family; the host reads
 * back one small record.  admit_dev: int32 [n] or NULL; window b's code: 0 admitted, 1 counts exceed capacities, 2 / 3 range edge (vertex index /
 * poses further apart than bw_max), 4 prior edge vertex index, 5 / 6 SE3 edge (as 2 / 3); written for every window, admitted batch or not.
 * A batch with a refused window is LOC_ERR_INVALID (loc_last_error: loc_window_upload's words for the code of the LOWEST refused window, and
 * that window's index): nothing is copied, and the previous resident batch stays exactly as it was and still solves.  An admitted batch is
 * copied device-to-device, and the handle is in the state loc_window_upload of the same arrays would have left — every resident entry works
 * unchanged — with one difference: only the chain family's verdicts (LOC_WINDOW_KERNEL_CHAIN3 / _WAVE3, _WAVE6, _WAVE6S, _CHAIN) are taken on the
 * device.  A forest- or arrowhead-shaped batch (whose schedule / packed records loc_window_upload builds on the host) solves on the general
 * kernel, correctly; its covariances are classified by the first covariance call as for any upload.
 * Option "upload_dev_structures" = 1 removes that difference: a batch that is no chain then takes the two tests loc_window_upload runs next,
 * in its order and under its conditions (options "arrow3" / "tree", the forest threshold, translation-only values, no endpoint-1 lever arms
 * or full information matrices for a forest), on the device.  One further launch pair on hip_stream decides both and the host reads back one
 * more record.  An arrowhead batch gets its row order and packed records from a third launch (nothing is packed on the host); for a forest
 * batch — every window's counts and used index rows equal window 0's — the host fetches window 0's counts and index rows, ONE window's, and
 * builds the schedule from them.  Kernel, covariance pass and solve bits are loc_window_upload's; so are the resident entries' answers
 * (loc_window_prune_resident refuses an ARROW3 batch).  hip_stream is then synchronised once or twice more.  Still on the host only: the
 * topology cache (every upload is analysed), loc_window_set_endpoint1_offsets / _set_prior_information (host arrays), and — unless the next
 * option is set — forest batches whose windows differ in topology (the general kernel).
 * Option "upload_dev_forest_groups" = 1 (with "upload_dev_structures" = 1 and "forest_groups" = 1) takes loc_window_upload's last test as well:
 * a batch the two tests above leave — no chain, no arrowhead, not of one topology — that "forest_groups" admits (its rule, unchanged) is
 * grouped by topology on the device: one wave per window hashes the window's topology key and finds the lowest window of that hash, compares
 * its key with that window's, and a one-workgroup scan numbers the groups by first appearance.  The host reads back one record, then the
 * window -> group map (4 bytes per window) and ONE window per group (counts and used index rows), builds the groups' schedules from those and
 * sends the block loc_window_upload sends, byte for byte.  A batch loc_window_upload would refuse to group (a window with fewer than 2 poses,
 * a cycle, two EdgeSE3 factors on one pair) solves on the general kernel, as there.  A hash collision (see "upload_dev_groups_hash_bits")
 * fetches the counts and index tables and groups on the host: the answer never depends on the hash.  The schedules themselves are still built
 * on the host.
 * Synchronisation: hip_stream is synchronised ONCE for the record (work the caller queued on it before the call — a kernel that writes the
 * arrays — is seen), and an admitted batch waits for the previous batch's resident work and for its own copies: like loc_window_upload the call
 * returns when the arrays are free again.  The host copies of the integer tables (the counts, and the mirror of option "resident_slide") are
 * fetched from the device by the first entry that reads them.
 * Timing: the pass's two launches are bracketed by the events loc_window_last_covariance_ms reads, as the slides' launches are (when option
 * "upload_dev_structures" adds launches the closing event is recorded again behind the last of them: the figure then spans admission, the
 * device-to-device copy and the structure / pack / grouping launches).  After the
 * call — a REFUSED one included — loc_window_last_covariance_ms reports the admit pass, no longer the previous batch's last covariance or
 * slide launch: read that figure before calling. */
int loc_window_upload_dev(loc_window* w, void* hip_stream, int64_t n_instances, const void* counts_dev, const void* poses_dev,
                          const void* r_idx_dev, const void* r_val_dev, const void* p_idx_dev, const void* p_val_dev,
                          const void* s_idx_dev, const void* s_val_dev, void* admit_dev);
int loc_window_solve_resident(loc_window* w, void* hip_stream);
int loc_window_download(loc_window* w, double* poses, double* result);
void* loc_window_poses_device(loc_window* w);   /* double [B][nv_max][12] */
void* loc_window_result_device(loc_window* w);  /* double [B][8] */
int loc_window_timing_begin(loc_window* w, int32_t max_launches);
int loc_window_timing_end(loc_window* w, int32_t* n_launches, double* total_ms, double* avg_ms);
/* Marginal pose covariances of CHAIN windows, of ARROWHEAD and FOREST batches and (option "covariance_general") of windows of any structure: for window b with estimate x, H = sum_e J_e^T (rho'_e Omega_e) J_e evaluated AT x
 * (rho'_e = 1 / (1 + chi2_e) on every range edge and on every EdgeSE3 whose robust flag is set — g2o's robustInformation without rho''; priors
 * not robustified; range Jacobians in the handle's mode, loc_window_set_jacobian; no LM damping), in g2o VertexSE3's minimal coordinates
 * [dt (body frame), dq_xyz] applied as x * fromVectorMQT(d); Sigma_i = [H^-1]_ii.  Unlike g2o's computeMarginals (which re-factors the H of the
 * last linearisation, one step behind x) the result is a function of the returned estimate alone.  A coordinate whose diagonal entry of H is
 * exactly 0 (a rotation without lever arm or rotation prior; every rotation of a translation-only batch) is excluded: its rows / columns are 0
 * and its bit is set in the mask.  A window whose block Cholesky meets a pivot that is not finite or not positive (the solve kernels' test), or
 * that is at most 1e-11 of its coordinate's diagonal entry of H (numerically singular: a rank-deficient H leaves pivots of rounding size and
 * either sign — e.g. a window that ranges ONE anchor per pose, as every configuration under cfg/ does: 2T - 1 rank-one terms for 3T translations),
 * gets LOC_ERR_SINGULAR and NaN in all its blocks; the other windows are not affected.  Same host layouts as loc_window_solve_host:
 *   cov    double [n][nv_max][36]  row-major 6x6 per pose slot (slots >= nv: 0)
 *   mask   int32  [n][nv_max]      excluded coordinates, bits 0-5 = tx ty tz qx qy qz
 *   status int32  [n]              LOC_OK or LOC_ERR_SINGULAR (that window's blocks NaN)
 * Covered (no endpoint-1 lever arms: the handle has none set, loc_window_set_endpoint1_offsets(w, 0, NULL)), LOC_ERR_UNSUPPORTED with nothing
 * written otherwise; tested in this order:
 *   - chains (nv_max <= 64): every pose-to-pose edge of every window, range or EdgeSE3, joins consecutive slots (several per pair, a missing
 *     link, any edge order);
 *   - arrowheads (anchor self-calibration: a tag trajectory whose poses range to 1 .. 12 unknown nodes, the window's LAST pose slots), iff the
 *     handle would solve the batch on arrow3_lm_kernel: option "arrow3" admits it (-1, the default: handles with nv_max > 64 only; 1: whenever
 *     the batch qualifies; 0: never), the batch is translation-only (no EdgeSE3, identity rotations, zero lever arms, priors without rotation
 *     information) and has that kernel's structure (at most one edge per pair of consecutive chain poses, every other pose-to-pose edge ends in
 *     the border; its anchor, record and LDS limits).  Any nv_max that kernel takes.  3x3 blocks: every rotation bit is set.  The unknown
 *     nodes' covariances are the blocks of their pose slots;
 *   - forests (nv_max <= 64), iff the handle would solve the batch on a forest kernel: option "tree" != 0, n at least the forest threshold (256 windows, or
 *     the chain threshold where loc_window_set_chain_threshold lowered it: 1 serves a single window), every window the same counts and index
 *     tables, 2 <= nv <= 64, and the pose-to-pose edges form a forest (several edges per pair, either direction, several trees, isolated
 *     poses).  Always 6x6 blocks.  A tree that no range, prior or lever arm ties to the world is singular (LOC_ERR_SINGULAR for its window);
 *   - forests of DIFFERING topologies (nv_max <= 64), only after the one-topology test has declined the batch and only with options
 *     "forest_groups" and "forest_groups_covariance" both 1, iff the handle would solve the batch on LOC_WINDOW_KERNEL_TREE_GROUPS: option "tree"
 *     neither 0 nor 2, n at least the forest threshold, no table of full information matrices, every window a forest of 2 <= nv <= 64 poses with
 *     at most one EdgeSE3 per pair of poses.  The windows are grouped by topology (anchor numbers and robust flags do not count) and every window
 *     is computed by the forest pass's arithmetic on its group's schedule: the bits a one-topology batch of that group's windows gets.  The
 *     launch's LDS is the largest group's: one 64-pose group puts every window of the batch at 60 KB (two windows per CU).
 *     loc_window_covariance_resident: a batch that loc_window_upload put on the grouped solve path walks the groups block already on the device
 *     (no copy-back, asynchronous); any other resident batch is classified by the first call as below and builds a block of its own;
 *   - with loc_window_set_option(w, "covariance_general", 1) — default 0: the tests above and nothing else, bit for bit — ANY batch the
 *     tests above leave: chains and forests of more than 64 poses, ragged or mixed batches (another graph in every window), 6-DoF arrowheads,
 *     windows with loops (an EdgeSE3 or a range that closes a cycle), any nv_max the handle takes.  Batches the tests above take keep their
 *     kernels and their bits.  Always 6x6 blocks (a translation-only window gets its rotation bits from the exactly-zero rule).  One workgroup
 *     per window: a block LDL^T with selected inversion on the ENVELOPE of the matrix IN THE CALLER'S POSE ORDER — pose slot i keeps the
 *     blocks from the smallest slot an edge joins it to up to itself; there is no reordering, so work and memory depend on the slot order as
 *     with loc_window_set_ordering(natural): a star packed leaves-first (as loc_node_* packs its key-frame windows) costs 2n - 1 blocks, the
 *     same star packed key-first n (n + 1) / 2.  The envelopes live in a device workspace of the handle, allocated on first use and grown on
 *     demand (a failed allocation is LOC_ERR_HIP); loc_window_covariance_plan reports its size beforehand.
 *     Windows with endpoint-1 lever arms stay LOC_ERR_UNSUPPORTED under either value of the option.
 *     A handle with full-information priors (loc_window_set_prior_information) is served by this pass ALONE, whatever its batch's structure:
 *     items 1 to 3 read p_val's diagonal and decline it, so with the option at 0 its covariance calls are LOC_ERR_UNSUPPORTED.
 * Stateless: does not change the handle's resident batch, last kernel kind / ms, topology cache or options.  Synchronous.  Small calls (inputs
 * and outputs within the 4 MiB staging block) travel as loc_window_solve_host's small ones do; larger ones stage through a device block of
 * their own — unlike a large loc_window_solve_host they leave the resident batch intact. */
/* The marginal prior of a dropped pose ("The marginal prior of a dropped pose"): what a sliding window keeps of its oldest pose
 * instead of throwing away everything that pose's factors knew (the reference's robot.cpp:92-98).  TRANSLATION-ONLY batches.  For window b,
 * d = drop[b], m = the one pose that pose-to-pose ranges join to d, x = poses: the factors with d as an endpoint (ranges to anchors, ranges
 * between d and m — several allowed, either direction —, priors on d) are linearised at x by the covariance definition (rho' = 1 / (1 + chi2)
 * on ranges, the handle's Jacobian mode, priors analytic and not robust, with their full matrix when loc_window_set_prior_information has set
 * one — which makes the call recursive: the prior a slide produced is a removed factor of a later slide); d's exactly-zero-diagonal coordinates
 * are excluded, H_dd is factored under both pivot tests of the covariance passes, and
 *   Lambda = H_mm - H_md H_dd^-1 H_dm (symmetrised),  gamma = g_m - H_md H_dd^-1 g_d.
 * Lambda is positive semi-definite and usually rank-deficient (one rank-1 smoothness link passes on one direction), so the pivot rule is not
 * reused on it: of its symmetric eigen-decomposition the pairs with lambda_k > 1e-11 lambda_max are kept.  Same host layouts as
 * loc_window_solve_host (poses is not written), the handle's anchors and Jacobian mode; stateless and synchronous, the resident batch is left alone.
 *   drop   int32  [n]      the pose slot to marginalise out, in [0, nv_b)
 *   slot   int32  [n]      the pose the prior sits on (m); -1: none
 *   prior  double [n][48]  Z^-1 as R(9), t(3), then the information 6x6 row-major (top-left 3x3 = sum of the kept lambda_k v_k v_k^T, zeros
 *                          elsewhere): an s_val row's layout = a p_val row's [0..11] followed by a loc_window_set_prior_information row.
 *                          Z^-1 = (I, e0 - t_m), so that toVectorMQT(Z^-1 X_m) = e0 and EdgeSE3Prior(Z, information) on m has gradient gamma and
 *                          Hessian Lambda at x: the removed factors' quadratic with d minimised out
 *   grad   double [n][6]   gamma (rotation entries 0)
 *   shift  double [n][6]   e0 = sum over the kept pairs of (v_k^T gamma / lambda_k) v_k: the minimum-norm solution of Lambda e0 = gamma
 *   rank   int32  [n]      eigenpairs kept
 *   status int32  [n]      LOC_OK or LOC_ERR_SINGULAR
 * A failed pivot of H_dd (the removed factors do not determine d: e.g. one anchor range alone) is LOC_ERR_SINGULAR for that window with slot =
 * m, information, grad and shift exact zeros, Z^-1 = X_m^-1 and rank 0 — zeros, not NaN, on purpose: the row is an input of the next solve,
 * and a zero-information prior IS the reference's plain drop.  A dropped pose without a neighbour: slot -1, zeros, identity Z^-1, LOC_OK
 * (whatever its own factors are).  Sums over edges run in edge order (ranges, then priors): the same bits on every run and for every position
 * of a window in the batch.
 * Checked on the host before anything is launched, nothing written on failure: LOC_ERR_INVALID for a drop slot outside [0, nv_b) (and for what
 * loc_window_solve_host refuses); LOC_ERR_UNSUPPORTED when endpoint-1 lever arms are set, when the batch is not translation-only (no EdgeSE3,
 * identity rotations, zero lever arms, priors with identity measurement rotation and no rotation information; with a full-matrix table: the
 * rotation rows and columns of EVERY matrix of the table exactly 0), or when pose-to-pose edges join some window's dropped pose to more than one
 * other pose (a marginal over several poses is not a unary prior; anchor self-calibration arrowheads are such windows).  6-DoF windows are out on
 * purpose.  loc_window_last_covariance_ms reports the pass's kernel time. */
int loc_window_marginal_prior_host(loc_window* w, int64_t n, const int32_t* counts, const double* poses, const int32_t* r_idx, const double* r_val,
                                   const int32_t* p_idx, const double* p_val, const int32_t* s_idx, const double* s_val, const int32_t* drop,
                                   int32_t* slot, double* prior, double* grad, double* shift, int32_t* rank, int32_t* status);
int loc_window_covariance_host(loc_window* w, int64_t n, const int32_t* counts, const double* poses,
                               const int32_t* r_idx, const double* r_val, const int32_t* p_idx, const double* p_val,
                               const int32_t* s_idx, const double* s_val, double* cov, int32_t* mask, int32_t* status);
/* The same for the uploaded batch at loc_window_poses_device()'s current content (after loc_window_solve_resident: the solved poses),
 * asynchronous on hip_stream (NULL = the handle's own stream; it waits for the last resident launch), into caller-owned device arrays of the
 * layouts above.  LOC_ERR_INVALID before the first resident solve of an upload.  The batch's structure is checked once per upload: an upload
 * that loc_window_upload classified as a chain or as a forest (whose schedule, already on the device, the pass walks) needs nothing more;
 * for any other upload the first call copies the uploaded tables back, classifies them (chain, then arrowhead and forest under the rules above,
 * into tables of the covariance's own, then the envelope pass where option "covariance_general" is 1) and is synchronous.  A batch held by
 * the envelope pass is classified again (one more synchronous call) when option "arrow3", option "tree" or the forest threshold has changed
 * since: the resident batch always takes the pass loc_window_covariance_host would take for the same tables. */
int loc_window_covariance_resident(loc_window* w, void* hip_stream, void* cov_dev, void* mask_dev, void* status_dev);
/* What the envelope pass (option "covariance_general") would allocate for this batch, from the structure alone: no device, no handle.
 * counts / r_idx / s_idx as loc_window_solve_host takes them (r_idx may be NULL when caps->nr_max is 0, s_idx likewise).
 *   blocks_max       the largest envelope of the batch in 6x6 blocks: over a window's pose slots i, the sum of i - first(i) + 1, first(i) = the
 *                    smallest slot a pose-to-pose edge (a range between two poses, an EdgeSE3) joins to slot i, i itself without one
 *   workspace_bytes  n * ((blocks_max + nv_max) * 36 + nv_max * 6) * 8: every window's envelope, one column of it and diag(H)
 * so that a caller can choose a slot order, or refuse, before touching the device.  LOC_ERR_INVALID: a count beyond the capacities or an
 * edge index outside its window. */
int loc_window_covariance_plan(const loc_window_caps* caps, int64_t n, const int32_t* counts, const int32_t* r_idx, const int32_t* s_idx,
                               int64_t* blocks_max, size_t* workspace_bytes);
/* Joint marginals: the calls above, and with them the cross blocks [H^-1]_ij of requested pairs of pose slots — what g2o's computeMarginals
 * returns for a list of block index pairs.  Same H, coordinates, exclusion rule and pivot rule, same coverage and dispatch as
 * loc_window_covariance_* (LOC_ERR_UNSUPPORTED with nothing written otherwise); every pass serves every pair.  The pair tables are HOST arrays
 * in both variants:
 *   npair_max    pair slots per window (0: no pairs — the call is loc_window_covariance_*, the pair arguments and cross may be NULL)
 *   pair_counts  int32 [n]                 0 <= pair_counts[b] <= npair_max
 *   pairs        int32 [n][npair_max][2]   pose slots (i, j) of window b, both in [0, nv_b); (i, i), (j, i) next to (i, j) and duplicates are allowed
 *   cross        double [n][npair_max][36] cross[b][p] = [H^-1]_ij, row-major 6x6, rows: pose i's coordinates, columns: pose j's
 * Rows of coordinates excluded in pose i and columns of coordinates excluded in pose j are 0 (3x3 passes: every rotation row / column).  (i, i)
 * has the bits of cov[b][i]; (j, i) is the exact transpose of (i, j) (one is computed and transposed), duplicates have equal bits.  Two poses
 * that nothing connects (different trees of a forest, an isolated pose) give exact zeros.  A LOC_ERR_SINGULAR window has NaN in all its
 * requested blocks; slots p >= pair_counts[b] are written as 0.  Every pair is checked on the host before anything is launched: a count or a
 * slot out of range is LOC_ERR_INVALID with nothing written.  cov, mask and status are those of the plain call (chains, arrowheads and
 * forests: bit for bit).  On the envelope pass a requested pair counts as one more pose-to-pose edge of the envelope (first(max(i, j)) <=
 * min(i, j)): the workspace grows by the blocks that adds, loc_window_joint_covariance_plan reports it.
 * _resident: cross_dev is a device array like cov_dev; the pair tables are copied to a device table of the handle before the launch and the
 * caller's arrays are not read after the call returns (a call may wait for the previous joint call's copy).
 * _plan: loc_window_covariance_plan for the envelope with the pairs; without pairs its results are loc_window_covariance_plan's.
 * LOC_ERR_INVALID also for a pair count or a pair's slot out of range. */
int loc_window_joint_covariance_host(loc_window* w, int64_t n, const int32_t* counts, const double* poses,
                                     const int32_t* r_idx, const double* r_val, const int32_t* p_idx, const double* p_val,
                                     const int32_t* s_idx, const double* s_val,
                                     int32_t npair_max, const int32_t* pair_counts, const int32_t* pairs,
                                     double* cov, int32_t* mask, int32_t* status, double* cross);
int loc_window_joint_covariance_resident(loc_window* w, void* hip_stream,
                                         int32_t npair_max, const int32_t* pair_counts_host, const int32_t* pairs_host,
                                         void* cov_dev, void* mask_dev, void* status_dev, void* cross_dev);
int loc_window_joint_covariance_plan(const loc_window_caps* caps, int64_t n, const int32_t* counts, const int32_t* r_idx, const int32_t* s_idx,
                                     int32_t npair_max, const int32_t* pair_counts, const int32_t* pairs, int64_t* blocks_max, size_t* workspace_bytes);
/* The pass that served the LAST loc_window_covariance_* / loc_window_joint_covariance_* call of this handle that launched, host path or
 * resident (a refused call leaves it as it was; LOC_WINDOW_COV_NONE before the first): under option "covariance_general" a caller cannot
 * tell otherwise whether a structured pass or the envelope pass computed a batch. */
enum { LOC_WINDOW_COV_NONE = 0, LOC_WINDOW_COV_CHAIN3 = 1 /* chains, 3x3 blocks */, LOC_WINDOW_COV_CHAIN6 = 2 /* chains, 6x6 blocks */, LOC_WINDOW_COV_ARROW = 3,
       LOC_WINDOW_COV_FOREST = 4 /* forests of one shared topology */, LOC_WINDOW_COV_ENVELOPE = 5 /* option "covariance_general" */,
       LOC_WINDOW_COV_FOREST_GROUPS = 6 /* forests of differing topologies: options "forest_groups" + "forest_groups_covariance" */ };
int loc_window_last_covariance_kind(const loc_window* w, int32_t* kind);
/* kernel time of the last covariance, marginal-prior or slide launch(es) of this handle (HIP events on its stream; a resident launch is
 * waited for), milliseconds */
int loc_window_last_covariance_ms(loc_window* w, double* ms);
/* The resident fixed-lag slide ("The resident slide"): drop the oldest pose of every uploaded window, carry its marginal prior,
 * append the newest pose and its factors — on the device, where the batch lives.  Needs loc_window_set_option(w, "resident_slide", 1) BEFORE
 * loc_window_upload (the upload then keeps a host mirror of counts, r_idx and p_idx; with 0, the default, an upload does what it always did
 * and this call is LOC_ERR_INVALID).  All inputs are HOST arrays; every output is a caller-owned DEVICE array and may be NULL.  Asynchronous
 * on hip_stream (NULL = the handle's own stream): it waits for the last resident launch, the caller's arrays are copied to a page-locked
 * block of the handle before the call returns (never read afterwards) and travel from there in stream order.
 *   drop_oldest  int32  [n]                  non-zero: window b drops slot 0; 0: it only grows; NULL: every window drops
 *   new_pose     double [n][12]              the appended pose, R(9) = identity, t(3)
 *   nr_new_max, new_r_counts [n], new_r_idx [n][nr_new_max][2], new_r_val [n][nr_new_max][5]   the appended range rows (r_idx / r_val layouts)
 *   np_new_max (may be 0), new_p_counts [n], new_p_val [n][np_new_max][18]                      the appended prior rows, all on the new pose
 *   slot_dev int32 [n], prior_dev double [n][48], rank_dev int32 [n], status_dev int32 [n]      loc_window_marginal_prior_host's layouts
 * Per window b, with x = loc_window_poses_device()'s content (the last resident solve's estimates):
 *   1. drop_oldest[b] != 0: the marginal prior of slot 0 at x — marginal_prior_kernel itself, with the handle's Jacobian mode and table: the
 *      bits loc_window_marginal_prior_host(.., drop = 0) returns for the same tables.  Slot 0 goes, with every range row that has it as an
 *      endpoint and every prior row on it (and that row of the table); the other rows keep their order; moving slot indices decrease by 1
 *      (anchor codes -1 - a stay); poses 1 .. nv - 1 move to 0 .. nv - 2.  If the marginal's slot >= 0 its row becomes prior row 0, on the new
 *      slot 0, in front of the kept priors (a LOC_ERR_SINGULAR marginal's zero-information row included): p_val[0..11] = prior[0..11],
 *      p_val[12..17] = the information's diagonal, table row = the information.
 *   2. drop_oldest[b] == 0: nothing is removed (a window grows to its lag); outputs slot -1, 48 zeros, rank 0, LOC_OK.
 *   3. new_pose[b] becomes the last slot s; then new_r_counts[b] range rows and new_p_counts[b] prior rows follow the kept ones.  Indices are
 *      in the NEW numbering: v0 is s or s - 1, v1 is s, s - 1 or an anchor code; a pose-to-pose row joins s - 1 and s; rows are listed in the
 *      order of their later pose (a row on s - 1 alone never after a row that names s).  The prior rows sit on s; their table row is
 *      diag(p_val[12..17]).
 *   4. the input estimates of the next resident solve AND loc_window_poses_device() become x's kept poses followed by new_pose; counts change
 *      on the device and in the host's mirror.
 *   5. a handle without a table of full information matrices gets one at its first slide ([batch][np_max][36]; every existing prior's row is
 *      diag(p_val[12..17])) and from then on behaves as after loc_window_set_prior_information.
 * After the call the handle is in the state loc_window_upload of the slid tables with that table set would leave: the kernel kind, the
 * covariance pass, the anchors it references, the joint call's counts.  A resident solve, (joint) covariance or download after it sees the
 * slid batch.  loc_window_last_covariance_ms reports the two launches (marginal pass + slide kernel).
 * Everything is checked on the host before anything is launched or changed.  LOC_ERR_INVALID: option "resident_slide" was 0 at upload time;
 * nothing uploaded; no resident solve since the upload; a table of full matrices that describes fewer windows than are resident; a new count
 * outside [0, *_new_max]; a new index outside rule 3; a slid window beyond nv_max, nr_max or np_max (counted from the mirror); a window with
 * nv = 0.  LOC_ERR_UNSUPPORTED: the resident batch's verdict is not LOC_WINDOW_KERNEL_CHAIN3 (an ordered translation-only chain, decided at
 * upload; an ordered chain minus slot 0 plus a last slot joined to its predecessor alone is an ordered chain, so the verdict survives);
 * endpoint-1 lever arms; a table with rotation entries; a new row that is not translation-only (a non-identity rotation, a non-zero lever
 * arm, rotation information). */
int loc_window_slide_resident(loc_window* w, void* hip_stream, const int32_t* drop_oldest, const double* new_pose,
                              int32_t nr_new_max, const int32_t* new_r_counts, const int32_t* new_r_idx, const double* new_r_val,
                              int32_t np_new_max, const int32_t* new_p_counts, const double* new_p_val,
                              void* slot_dev, void* prior_dev, void* rank_dev, void* status_dev);
/* loc_window_slide_resident with its per-window inputs in DEVICE arrays, and the admission of every window on the device.  Layouts and rules
 * 1 to 5 are those of loc_window_slide_resident (above; DESIGN.md §2, "The resident slide").  drop_oldest_dev may be NULL: every window drops.
 * Every output may be NULL; admit_dev int32 [n] gets one LOC_SLIDE_ADMIT_* code per window.
 * How the inputs are read: the caller's arrays are device memory and the kernels read them directly, in stream order on hip_stream (NULL = the
 * handle's own stream) — no page-locked copy, no hipMemcpy.  The caller keeps them alive and unchanged until the stream has passed the call,
 * orders its own writes to them before the call (the handle's stream does not wait for any other), and they may not alias the handle's
 * tables (loc_window_poses_device() among them) or the outputs.  The call makes no pass over per-window data on the host and does not
 * synchronise; the exceptions are the one-time allocations loc_window_slide_resident also makes (the marginal pass's block at a handle's first
 * slide; a new table of full information matrices, after waiting for the last resident launch).
 * Checked on the host, with nothing launched or changed, exactly as by loc_window_slide_resident — LOC_ERR_INVALID: option "resident_slide"
 * was 0 at upload time; nothing uploaded; no resident solve since the upload; a table of full matrices that describes fewer windows than are
 * resident; a NULL new_pose_dev, a negative capacity or a NULL array under a positive one.  LOC_ERR_UNSUPPORTED: the resident batch's verdict is
 * not LOC_WINDOW_KERNEL_CHAIN3; endpoint-1 lever arms; a table with rotation entries.
 * Checked on the device, per window, by the wave that slides it: admit[b] = LOC_SLIDE_ADMIT_OK, or the first rule the window breaks.  THERE IS NO
 * BATCH-WIDE REFUSAL BEFORE LAUNCH: a refused window is left exactly as it was (counts, every table row, poses, the next solve's input
 * estimates) and reports slot -1, 48 zeros, rank 0 and status LOC_ERR_INVALID (codes 1 to 6) or LOC_ERR_UNSUPPORTED (code 7), while the other
 * windows of the batch slide normally and report what loc_window_slide_resident reports.  A first slide that creates the table (rule 5)
 * creates it for the refused windows as well: their rows become diag(p_val[12..17]).  Anchor codes are admitted against the anchor table's
 * size at call time.  The verdict of a window does not depend on its position in the batch.
 * Afterwards the handle is in the state loc_window_slide_resident leaves, except that its host mirror of counts, r_idx and p_idx is stale:
 * the next call that needs it (loc_window_slide_resident, loc_window_joint_covariance_resident with pairs, loc_window_set_anchors) first waits
 * for the resident work and fetches it.  loc_window_solve_resident, loc_window_covariance_resident, loc_window_download and
 * loc_window_download_tables do not need it, so K cycles of (solve, slide) queue on a stream without a host round trip.
 * loc_window_last_covariance_ms reports the two launches. */
enum {
    LOC_SLIDE_ADMIT_OK = 0,
    LOC_SLIDE_ADMIT_NO_POSES = 1,         /* the window has nv = 0 */
    LOC_SLIDE_ADMIT_COUNT = 2,            /* a new count outside [0, *_new_max] */
    LOC_SLIDE_ADMIT_INDEX = 3,            /* a new range index outside rule 3 (loc_window_slide_plain_resident_dev: or a new EdgeSE3 row not on {s - 1, s}) */
    LOC_SLIDE_ADMIT_NV_MAX = 4,           /* the slid window exceeds nv_max */
    LOC_SLIDE_ADMIT_NR_MAX = 5,           /* ... nr_max */
    LOC_SLIDE_ADMIT_NP_MAX = 6,           /* ... np_max */
    LOC_SLIDE_ADMIT_NOT_TRANSLATION = 7,  /* a new row that is not translation-only: a non-identity rotation, a lever arm, rotation information */
    LOC_SLIDE_ADMIT_NS_MAX = 8,           /* loc_window_slide_plain_resident_dev: the slid window exceeds ns_max */
    LOC_SLIDE_ADMIT_PAIRS = 9             /* loc_window_slide_plain_resident_dev: the new rows break the pair rule of the resident verdict */
};
int loc_window_slide_resident_dev(loc_window* w, void* hip_stream, const void* drop_oldest_dev, const void* new_pose_dev,
                                  int32_t nr_new_max, const void* new_r_counts_dev, const void* new_r_idx_dev, const void* new_r_val_dev,
                                  int32_t np_new_max, const void* new_p_counts_dev, const void* new_p_val_dev,
                                  void* slot_dev, void* prior_dev, void* rank_dev, void* status_dev, void* admit_dev);
/* The resident slide for 6-DoF chain windows: the reference's PLAIN DROP ("The plain drop for 6-DoF chain windows").  What
 * Robot::new_vertex does with its oldest pose (robot.cpp:92-98): the pose is thrown away with every factor on it and NOTHING is carried — no
 * marginal pass, no inserted prior row, no table of full information matrices.  It serves the resident verdicts LOC_WINDOW_KERNEL_CHAIN,
 * _WAVE6 and _WAVE6S (the ordered 6-DoF chain verdicts of loc_window_upload: IMU rotation priors, lever arms, EdgeSE3 factors between
 * consecutive poses), which loc_window_slide_resident(_dev) refuse.  Needs option "resident_slide" = 1 at upload, like its siblings.
 * Every per-window array is a DEVICE array in loc_window_slide_resident_dev's layouts and under its rules (read in stream order, kept alive
 * and unchanged by the caller until the stream has passed the call, no aliasing of the handle's tables or the outputs); in addition
 *   ns_new_max (may be 0), new_s_counts int32 [n], new_s_idx int32 [n][ns_new_max][4], new_s_val double [n][ns_new_max][48]
 * the appended EdgeSE3 rows in the s_idx / s_val layouts.  New priors sit on the new slot: there is no index array for them.
 * drop_oldest_dev may be NULL: every window drops.  status_dev int32 [n] and admit_dev int32 [n] may be NULL.  Asynchronous on hip_stream
 * (NULL = the handle's own stream), ordered after the last resident launch; no pass over per-window data on the host, no copy, no
 * synchronisation, no allocation.
 * Per window b, with x = loc_window_poses_device()'s content:
 *   1. drop_oldest[b] != 0: slot 0 goes, with every range row that has it as an endpoint, every prior row on it and every EdgeSE3 row that has
 *      it as vi or vj; the kept rows keep their order; every moving slot index decreases by 1 (anchor codes -1 - a stay, s_idx[.][2..3]
 *      travel as they are); poses 1 .. nv - 1 move to 0 .. nv - 2, all 12 doubles.
 *   2. drop_oldest[b] == 0: nothing is removed.
 *   3. new_pose[b] (any rotation) becomes the last slot s; the new range rows follow the kept ones under rule 3 of loc_window_slide_resident;
 *      the new prior rows go on s; the new EdgeSE3 rows must have {vi, vj} = {s - 1, s} in either order, with s - 1 >= 0 and bw_max >= 1.
 *      Lever arms, rotations and rotation information are allowed.
 *   4. loc_window_poses_device() AND the input estimates of the next resident solve become the kept poses followed by new_pose; counts[b]
 *      changes, [3] included.
 * Checked on the host, with nothing launched or changed — LOC_ERR_INVALID as loc_window_slide_resident_dev; LOC_ERR_UNSUPPORTED: the resident
 * verdict is LOC_WINDOW_KERNEL_CHAIN3 (loc_window_slide_resident / loc_window_slide_resident_dev slide such a batch) or any verdict that is
 * not an ordered 6-DoF chain; endpoint-1 lever arms; a handle with a table of full information matrices.
 * Checked on the device, per window, by the wave that slides it: admit[b] = LOC_SLIDE_ADMIT_OK or the first rule broken, in the order 1, 2
 * (new_s_counts included), 3 (the EdgeSE3 index rule included), 4, 5, 6, 8, 9; code 7 is never produced.  LOC_SLIDE_ADMIT_PAIRS depends on the
 * resident verdict — _WAVE6: any new EdgeSE3 row, or more than one new pose-to-pose range row; _WAVE6S: more than one new EdgeSE3 row, or
 * more than one new pose-to-pose range row; _CHAIN: never.  A refused window is left exactly as it was and reports status LOC_ERR_INVALID
 * (codes 1 to 6 and 8) or LOC_ERR_UNSUPPORTED (code 9); the other windows slide and report LOC_OK.
 * Afterwards the handle keeps its verdict (an ordered chain minus slot 0 plus a last slot joined to its predecessor alone is an ordered
 * chain, and code 9 keeps the pair rule), the covariance pass is the chain pass again, and the host mirror is stale exactly as after
 * loc_window_slide_resident_dev.  loc_window_last_covariance_ms reports the launch. */
int loc_window_slide_plain_resident_dev(loc_window* w, void* hip_stream, const void* drop_oldest_dev, const void* new_pose_dev,
                                        int32_t nr_new_max, const void* new_r_counts_dev, const void* new_r_idx_dev, const void* new_r_val_dev,
                                        int32_t np_new_max, const void* new_p_counts_dev, const void* new_p_val_dev,
                                        int32_t ns_new_max, const void* new_s_counts_dev, const void* new_s_idx_dev, const void* new_s_val_dev,
                                        void* status_dev, void* admit_dev);
/* Rows from raw messages ("Rows from raw messages"): the step that turns ONE message per window into the window's newest pose
 * and its factors, on the device — Localization::addRangeEdge (localization.cpp:297-376: the outlier gate :306-313, sigma^2 :318-319, the
 * two-edge topology :327-340, the antenna lever arm :333-334), Robot::new_vertex (robot.cpp:75-110: the initial estimate :90, drop-oldest
 * :92-98), addImuEdge (:499-535), addLidarEdge (:462-496) and addTwistEdge with twist2transform (:438-459, :560-605).  One launch
 * (window_message_kernel.hip) writes exactly the arrays the two resident slides read, so (messages -> rows -> slide -> solve) queues on a
 * stream with nothing but the messages crossing to the device.  The rule is stated once, for host and device, in
 * localization_amd/csrc/message_rows.h.
 * Configuration, per handle (loc_window_set_message_config): trajectory_length in [1, nv_max]; maximum_velocity (:319); distance_outlier (:78;
 * <= 0 disables the gate); the antenna table antenna_xyz_host double [n_antenna][3] (:111-123; a message's `antenna` is 1-based, 0 = none),
 * copied to the device by the call.  The call also allocates the handle's own block of the eleven output arrays at batch capacity: no later
 * call allocates.  LOC_ERR_INVALID: a NULL handle or configuration, trajectory_length outside [1, nv_max], a maximum_velocity or
 * distance_outlier that is not a number, n_antenna < 0, n_antenna > 0 without a table.  Synchronous (waits for the last resident launch).
 * The message of window b, DEVICE arrays in one struct of pointers (n = the resident batch's windows):
 *   kind         int32 [n]       bit set: LOC_MSG_RANGE 1, LOC_MSG_IMU 2, LOC_MSG_LIDAR 4, LOC_MSG_TWIST 8.  Legal: 0 (no message), RANGE with
 *                                any subset of IMU / LIDAR, TWIST alone
 *   dt           double [n]      the message stamp minus the newest pose's stamp (:316, :442).  The caller keeps the stamps: the handle has
 *                                no per-window state for them
 *   anchor, antenna int32 [n], distance, distance_err float [n]     the range message (responder = anchor table index)
 *   imu          double [n][7]   q xyzw, then orientation_covariance[0], [4], [8]
 *   lidar_z      double [n]      the lidar height
 *   twist        double [n][42]  linear 3, angular 3, covariance 36 row-major
 * kinds_mask names the bits that may occur: kind and dt are always required, every other array exactly when its bit is in the mask (it may
 * be NULL otherwise and is then never read).
 * The output of window b, in the slides' layouts at the capacities LOC_MSG_NR_NEW / _NP_NEW / _NS_NEW — with nv the window's count, x its
 * newest solved pose (slot nv - 1 of loc_window_poses_device()), drop = (nv == trajectory_length) and s = nv - drop:
 *   drop_oldest[b] = drop; new_pose[b] = x (robot.cpp:90)
 *   RANGE  (the frame-id branch of :327 is always taken, as every cfg stream of the reference takes it)
 *          row 0 (s, -1 - anchor): measurement (double)distance, information 1 / ((double)distance_err)^2, lever arm antenna_xyz[antenna - 1]
 *          or zeros for antenna == 0; row 1 (s - 1, s): measurement 0, information 1 / (maximum_velocity dt / 3)^2, no lever arm — left out
 *          when s == 0
 *   IMU    first: new_pose's R = the quaternion's matrix (not normalised), t kept; one prior row Z^-1 = new_pose^-1, information
 *          (0, 0, 0, 1/c0, 1/c4, 1/c8)
 *   LIDAR  after IMU: new_pose.t[2] = lidar_z; one prior row Z^-1 = new_pose^-1, information (0, 0, 1/0.05, 0, 0, 0)
 *   TWIST  no range or prior row; one EdgeSE3 row (s - 1, s, 1, 0), Z^-1 of setRPY(w dt) / v dt as the node forms it, information
 *          (cov dt^2)^-1
 *   gate   a RANGE message with distance_outlier > 0 and nv == trajectory_length (the window is at its lag: the batch's statement of
 *          number_measurements > trajectory_length) is rejected when | ||x.t - anchor|| - (double)distance | > distance_outlier
 * verdict[b], by the first test that decides: LOC_MSG_NONE (kind == 0); LOC_MSG_INVALID (nv <= 0 or nv > trajectory_length; an illegal kind
 * or a bit outside kinds_mask; anchor outside the anchor table; antenna outside [0, n_antenna]; TWIST with s == 0); LOC_MSG_REJECTED (the
 * gate); LOC_MSG_INVALID (an information value that must be finite and positive and is not: distance_err == 0, dt == 0 with a row 1, a zero
 * or negative IMU covariance — STRICTER than the reference, which hands g2o an infinity); LOC_MSG_SINGULAR (the twist covariance times dt^2
 * has no inverse); LOC_MSG_APPENDED.  For every verdict but APPENDED the three counts are written as -1 — both slides then refuse that
 * window with LOC_SLIDE_ADMIT_COUNT and leave it exactly as it was — no row is written, and new_pose[b] is still x.  Rows at or beyond a
 * count are left unwritten.  Everything is bit for bit what message_rows.h gives on the host, except the rotation of a TWIST row with a
 * non-zero angular rate (sin and cos: DESIGN.md §3).
 * loc_window_message_rows_dev: build only, into caller-owned DEVICE arrays (verdict may be NULL).  Asynchronous on hip_stream (NULL = the
 * handle's own stream), ordered after the last resident launch; no host pass, no copy, no synchronisation, no allocation.  It serves every
 * resident verdict (it reads only counts and poses) and needs no option.  LOC_ERR_INVALID, with nothing launched: a NULL handle, no
 * configuration, nothing uploaded, no resident solve since the upload, kinds_mask with unknown bits, a NULL array under a mask bit (kind
 * and dt always), a NULL output other than verdict.
 * loc_window_push_messages_resident_dev: builds into the handle's own block, then calls the slide the resident verdict calls for on the
 * same stream — LOC_WINDOW_KERNEL_CHAIN3: loc_window_slide_resident_dev (with its marginal carry); _CHAIN / _WAVE6 / _WAVE6S:
 * loc_window_slide_plain_resident_dev.  Every host refusal of those slides is returned unchanged with NOTHING launched, the build included.
 * verdict_dev int32 [n], status_dev int32 [n] and admit_dev int32 [n] may be NULL.  Read verdict FIRST: a window with LOC_MSG_NONE or
 * _REJECTED shows admit code LOC_SLIDE_ADMIT_COUNT (and status LOC_ERR_INVALID), and that is not an error.  The slide's own per-window
 * refusals appear in admit_dev as they do today: LOC_SLIDE_ADMIT_NOT_TRANSLATION for an IMU message or a lever arm on a translation-only
 * batch, the capacities, the pair rule. */
enum { LOC_MSG_RANGE = 1, LOC_MSG_IMU = 2, LOC_MSG_LIDAR = 4, LOC_MSG_TWIST = 8 };
enum { LOC_MSG_NONE = 0, LOC_MSG_APPENDED = 1, LOC_MSG_REJECTED = 2, LOC_MSG_INVALID = 3, LOC_MSG_SINGULAR = 4 };
#define LOC_MSG_NR_NEW 2
#define LOC_MSG_NP_NEW 2
#define LOC_MSG_NS_NEW 1
typedef struct loc_window_message_config {
    int32_t trajectory_length;
    double maximum_velocity;
    double distance_outlier;
} loc_window_message_config;
typedef struct loc_window_messages {
    const void* kind;          /* int32 [n] */
    const void* dt;            /* double [n] */
    const void* anchor;        /* int32 [n] */
    const void* antenna;       /* int32 [n] */
    const void* distance;      /* float [n] */
    const void* distance_err;  /* float [n] */
    const void* imu;           /* double [n][7] */
    const void* lidar_z;       /* double [n] */
    const void* twist;         /* double [n][42] */
} loc_window_messages;
typedef struct loc_window_message_rows {
    void* drop_oldest;         /* int32 [n] */
    void* new_pose;            /* double [n][12] */
    void* new_r_counts;        /* int32 [n] */
    void* new_r_idx;           /* int32 [n][LOC_MSG_NR_NEW][2] */
    void* new_r_val;           /* double [n][LOC_MSG_NR_NEW][5] */
    void* new_p_counts;        /* int32 [n] */
    void* new_p_val;           /* double [n][LOC_MSG_NP_NEW][18] */
    void* new_s_counts;        /* int32 [n] */
    void* new_s_idx;           /* int32 [n][LOC_MSG_NS_NEW][4] */
    void* new_s_val;           /* double [n][LOC_MSG_NS_NEW][48] */
    void* verdict;             /* int32 [n], may be NULL */
} loc_window_message_rows;
int loc_window_set_message_config(loc_window* w, const loc_window_message_config* cfg, int32_t n_antenna, const double* antenna_xyz_host);
int loc_window_message_rows_dev(loc_window* w, void* hip_stream, int32_t kinds_mask, const loc_window_messages* msgs,
                                const loc_window_message_rows* out);
int loc_window_push_messages_resident_dev(loc_window* w, void* hip_stream, int32_t kinds_mask, const loc_window_messages* msgs,
                                          void* verdict_dev, void* status_dev, void* admit_dev);
/* The resident batch as it stands (a checkpoint; host arrays in loc_window_upload's layouts, n = the resident batch's windows; any pointer may
 * be NULL).  poses: the estimates the next resident solve starts from.  pinfo double [n][np_max][36]: the table of full information matrices;
 * LOC_ERR_INVALID when the handle has none.  Synchronous (waits for the last resident launch). */
int loc_window_download_tables(loc_window* w, int32_t* counts, double* poses, int32_t* r_idx, double* r_val, int32_t* p_idx, double* p_val,
                               int32_t* s_idx, double* s_val, double* pinfo);
/* Edge audit and outlier removal ("Edge audit and outlier removal"): the block Localization::solve() keeps after
 * optimizer.optimize() (localization.cpp:172-181) — with more than 100 active edges, every range edge whose chi2() exceeds 2.0 gets
 * setLevel(1) and is left out of every later initializeOptimization().  Two things: the chi2 of every edge of every window, and that rule
 * applied in place to the resident batch by the GPU.  Every structure, every handle state (endpoint-1 lever arms, a table of full
 * information matrices): no dispatch, no LOC_ERR_UNSUPPORTED but the one below.
 * Evaluated at x = the poses given (_host) or loc_window_poses_device()'s current content (_resident): a function of the returned estimate
 * alone, not of g2o's "last evaluated state".  chi2 of a row is BaseEdge::chi2() = e^T Omega e, NOT robustified:
 *   range    e = ||X0 o0 - p1|| - meas, p1 = X1 o1 / anchor + o1 with endpoint-1 lever arms set, X1.t / the anchor without; chi2 = e (info e).
 *            One arithmetic form whatever loc_window_set_jacobian says (the plain-CPU operation order of the numeric solves): the bits do not
 *            depend on the Jacobian mode.
 *   prior    e = toVectorMQT(Z^-1 X), W = diag(p_val[12..17]), or the row of loc_window_set_prior_information's table when one is set
 *   EdgeSE3  e = toVectorMQT(Z^-1 Xi^-1 Xj), Omega = the 6x6 of s_val; the robust flag does not enter
 * Outputs (any may be NULL):
 *   r_chi2 double [n][nr_max], p_chi2 double [n][np_max], s_chi2 double [n][ns_max]    slots at or beyond the window's count are written 0
 *   total  double [n]   the sum over all rows of the window
 *   active int32  [n]   (range rows with information != 0) + np + ns
 * LEVEL 1 IS INFORMATION EXACTLY 0.0: such a range row adds exact zeros to chi2, H and b in every kernel.  So a caller's own zero-information
 * range is at level 1: it is not counted in `active` and never flagged.  And result[b][0] of a later solve does not contain a removed row
 * (g2o's OptimizableGraph::chi2() would keep its stale last value).
 * loc_window_edge_chi2_host: host arrays in loc_window_solve_host's layouts (poses is not written), stateless and synchronous, the resident
 * batch is left alone; LOC_ERR_INVALID for what loc_window_solve_host refuses.
 * _resident calls: caller-owned DEVICE arrays, asynchronous on hip_stream (NULL = the handle's own stream), ordered after the last resident
 * launch and before the next one; nothing is read on the host, nothing synchronises, the host mirror of a slide stays as it is.
 * LOC_ERR_INVALID, with nothing launched or written: a NULL handle, nothing uploaded, no resident solve since the upload, a table of full
 * matrices that describes fewer windows than are resident.
 * loc_window_prune_resident (the reference: chi2_max = 2.0, min_edges = 100), per window at x:
 *   if active[b] > min_edges, every range row with information != 0 and chi2 > chi2_max gets removed[b][e] = 1 and r_val[b][e][1] = 0.0
 * Both comparisons are strict, as in the reference; a NaN chi2 compares false and stays in; the decision uses the active count from before any
 * removal of this call.  Nothing else changes: no other entry of any table, no count, no pose, not the next solve's input estimates, none of
 * the handle's verdicts (they read no range value).  removed int32 [n][nr_max]: 0 for rows not removed and for padding; n_removed int32 [n]:
 * the rows removed; either may be NULL.  Also LOC_ERR_INVALID: chi2_max NaN or negative, min_edges < 0.  LOC_ERR_UNSUPPORTED: the resident
 * batch's verdict is LOC_WINDOW_KERNEL_ARROW3 — that kernel solves from records packed at upload, which a store into r_val does not reach
 * (every other solve kernel and covariance pass reads r_val at launch); loc_window_edge_chi2_resident serves such a batch normally.
 * loc_window_last_covariance_ms reports the launch. */
int loc_window_edge_chi2_host(loc_window* w, int64_t n, const int32_t* counts, const double* poses, const int32_t* r_idx, const double* r_val,
                              const int32_t* p_idx, const double* p_val, const int32_t* s_idx, const double* s_val,
                              double* r_chi2, double* p_chi2, double* s_chi2, double* total, int32_t* active);
int loc_window_edge_chi2_resident(loc_window* w, void* hip_stream, void* r_chi2_dev, void* p_chi2_dev, void* s_chi2_dev,
                                  void* total_dev, void* active_dev);
int loc_window_prune_resident(loc_window* w, void* hip_stream, double chi2_max, int32_t min_edges,
                              void* removed_dev /* int32 [n][nr_max] */, void* n_removed_dev /* int32 [n] */);
/* Publish and path records of a resident batch ("Publish and path records of a resident batch"): what the reference does with
 * a window after every solve, on the device, in stream order, into the caller's DEVICE arrays.
 *   loc_window_publish_resident   Localization::publish()     localization.cpp:195-226 — the gate optimizer.chi2() < minimum_optimize_error
 *                                 (:199), Robot::current_pose() (robot.cpp:146-157), path->poses[trajectory_length / 2] (:220), tf::poseEigenToMsg
 *   loc_window_path_resident      Robot::vertices2path()      robot.cpp:61-72 (first = 0, count = T); the destructor's tail path[T/2 .. T-1]
 *                                 (localization.cpp:708-717: first = T / 2, count = T - T / 2 — loc_node_flush_tail's rows for one window)
 * A record is 7 doubles: x, y, z, qx, qy, qz, qw — the position and Eigen::Quaterniond(R) with tf::poseEigenToMsg's w >= 0 flip: the node's
 * 8-double rows without their stamp (stamps stay the caller's, as for the message entries).  The records are bitwise what the node forms from
 * the same pose.
 * With T = trajectory_length, a window holds the newest nv of the ring's T poses: path index i is window slot i - (T - nv), slot nv - 1 is path
 * index T - 1.  The T - nv oldest ring vertices (the reference's never-measured initial vertices) are not in the window: they are reported as
 * absent, not invented.  Per window b, with nv = counts[b][0] and chi2 = result[b][0] of loc_window_result_device() (what the node gates on):
 *   flags     int32  [n]     bit 0: published = 1 <= nv and chi2 < minimum_optimize_error (strict; a NaN chi2 is never published, +inf publishes
 *                            every other window); bit 1: the optimized pose, path index T / 2, is in the window (whatever the gate says)
 *   realtime  double [n][7]  the newest pose, slot nv - 1; written ONLY with bit 0
 *   optimized double [n][7]  path index T / 2; written ONLY with bits 0 and 1
 *   chi2      double [n]     result[b][0], always written (a caller who gates differently needs no second array)
 *   n_published int32 [1]    the windows with bit 0: zeroed on the stream before the launch, then summed by the kernel
 * Rows of unpublished windows are left exactly as the caller had them (the reference returns before it forms a pose, :201-205).
 * realtime, optimized, chi2 and n_published may each be NULL; flags may not.
 *   path      double [n][count][7]   path index first + k at [b][k]; written ONLY where present; no gate (the reference has none there)
 *   present   int32  [n][count]      1 where the window holds that path index, else 0
 * A window with nv > trajectory_length is the caller's inconsistency: its flags are 0, its path rows are all absent, and no record of it is
 * written (chi2[b] still is).
 * Both calls: asynchronous on hip_stream (NULL = the handle's own stream), ordered after the last resident launch and before the next one;
 * nothing is read on the host, nothing synchronises, the host mirror of a slide stays as it is (loc_window_edge_chi2_resident's contract).
 * Only counts, poses and result are read: every structural verdict and every handle state is served, nothing of the batch is written.
 * Publish AFTER the solve: between a slide and the next solve, slot nv - 1 holds the appended, unsolved pose and result the previous
 * solve's chi2; that call is not refused.
 * LOC_ERR_INVALID, with nothing launched or written: a NULL handle, nothing uploaded, no resident solve since the upload, trajectory_length
 * < 1 or > nv_max, a NaN minimum_optimize_error, first < 0, count < 1 or first + count > trajectory_length, a NULL flags_dev, path_dev or
 * present_dev.  loc_window_last_covariance_ms reports the launch. */
int loc_window_publish_resident(loc_window* w, void* hip_stream, double minimum_optimize_error, int32_t trajectory_length,
                                void* flags_dev, void* realtime_dev, void* optimized_dev, void* chi2_dev, void* n_published_dev);
int loc_window_path_resident(loc_window* w, void* hip_stream, int32_t trajectory_length, int32_t first, int32_t count,
                             void* path_dev, void* present_dev);

/* ================================================================================================
 * Node front-end — `class Localization` behind the ABI (one moving tag, its ring window, its anchors).
 * Same callbacks, same parameters, same gating as the reference; every solve() is one window-kernel launch.
 *   loc_node_create        Localization::Localization          localization.cpp:32-161 (+ Robot::init, robot.cpp:31-58)
 *   loc_node_add_range     Localization::addRangeEdge          localization.cpp:297-376
 *   loc_node_add_imu       Localization::addImuEdge            localization.cpp:499-535
 *   loc_node_add_pose      Localization::addPoseEdge           localization.cpp:254-290
 *   loc_node_add_twist     Localization::addTwistEdge          localization.cpp:438-459, 560-605
 *   loc_node_add_lidar     Localization::addLidarEdge          localization.cpp:462-496
 *   loc_node_add_rl_range  Localization::addRLRangeEdge        localization.cpp:378-436 (built only with -DRELATIVE_LOCALIZATION,
 *                                                              CMakeLists.txt:137; message uwb_reloc::uwbTalkData)
 *   loc_node_solve         Localization::solve + publish       localization.cpp:164-251
 *   loc_node_get_path      Robot::vertices2path                robot.cpp:61-72
 * add_* return 1 when the call ran a solve (out is filled), 0 when it did not, < 0 on error.
 * Poses are 8 doubles: stamp, x, y, z, qx, qy, qz, qw (the TUM order the reference logs, localization.cpp:630-642).
 * Limits of this kernel version: trajectory_length (x number of nodes with topic/relative_range) <= 1024 poses.
 * ============================================================================================== */
typedef struct loc_node loc_node;

typedef struct loc_node_config {
    int32_t trajectory_length;        /* robot/trajectory_length           localization.cpp:72 (no default) */
    double maximum_velocity;          /* robot/maximum_velocity (1.0)       :75 */
    double distance_outlier;          /* robot/distance_outlier (1.0)       :78 */
    int32_t maximum_iteration;        /* optimizer/maximum_iteration (20)   :65 */
    double minimum_optimize_error;    /* optimizer/minimum_optimize_error (1000)  :68 */
    int32_t publish_range, publish_pose, publish_twist, publish_lidar, publish_imu; /* publish_flag/...  :146-158 */
    int32_t has_relative_range;       /* topic/relative_range present: every node moves  :94 */
    int32_t jacobian;                 /* LOC_JAC_NUMERIC_G2O (default) = what the reference's EdgeSE3Range inherits from g2o
                                         (types_edge_se3range.h:45-74), or LOC_JAC_ANALYTIC (opt-in fast mode) */
    int32_t publish_relative_range;   /* publish_flag/relative_range  :158 */
} loc_node_config;

typedef struct loc_node_output {
    int32_t solved;                   /* a solve ran */
    int32_t published;                /* chi2 < minimum_optimize_error (localization.cpp:199-205) */
    double chi2;                      /* optimizer.chi2() */
    double realtime[8];               /* robots[self].current_pose()            :208 */
    double optimized[8];              /* path->poses[trajectory_length / 2]     :220 */
    int32_t outer_iterations, lm_trials;
} loc_node_output;

void loc_node_default_config(loc_node_config* c);
/* ids[n-1] is the moving tag (nodesId.back(), :89); pos_xyz = /uwb/nodesPos; antenna_xyz = /uwb/antennaOffset or NULL */
int loc_node_create(loc_node** out, int32_t device, const loc_node_config* cfg, int32_t n_nodes, const int32_t* ids,
                    const double* pos_xyz, int32_t n_antenna, const double* antenna_xyz);
int loc_node_destroy(loc_node* n);
int loc_node_add_range(loc_node* n, int32_t requester_id, int32_t responder_id, double stamp, float distance,
                       float distance_err, int32_t antenna, const char* frame_id, loc_node_output* out);
int loc_node_add_imu(loc_node* n, double stamp, const double* q_xyzw, const double* orientation_cov9,
                     const char* frame_id, loc_node_output* out);
int loc_node_add_pose(loc_node* n, double stamp, const double* pose_xyz_qxyzw, const double* cov36,
                      const char* frame_id, loc_node_output* out);
int loc_node_add_twist(loc_node* n, double stamp, const double* twist_lin_ang6, const double* cov36,
                       const char* frame_id, loc_node_output* out);
int loc_node_add_lidar(loc_node* n, double stamp, double z, const char* frame_id, loc_node_output* out);
/* uwbTalkData: time_stamp, rqstrId, rspdrId, d, (rqstr_vx, rqstr_vy, rqstr_vz).  Peer range with the fixed sigma_d = 0.054 m, the
 * responder's smoothness edge, and for a moving requester an EdgeSE3 from its previous pose with measurement
 * translate(dt * v) and information diag(1/sigma_v^2 x3, 0 x3), no robust kernel; solves when publish_relative_range. */
int loc_node_add_rl_range(loc_node* n, int32_t requester_id, int32_t responder_id, double stamp, double distance,
                          const double* requester_velocity_xyz, loc_node_output* out);
int loc_node_solve(loc_node* n, loc_node_output* out);
int loc_node_get_path(loc_node* n, int32_t node_id, double* out_T_by_8, int32_t capacity_poses);
int32_t loc_node_number_measurements(const loc_node* n);
/* Where the last solve's time went, milliseconds: [0] packing the window on the host, [1] the window solve call (copy in, launch, copy
 * out, synchronise), [2] of which the kernel: launch to completion on the host clock — HIP events around the kernel when LOCAMD_KERNEL_EVENTS=1 was
 * set when the node made its solver handle (they cost ~4 us per message).  The reference prints the same figure per solve (CPPTimer,
 * localization.cpp:166,191) */
int loc_node_last_timing(const loc_node* n, double* pack_solve_kernel_ms);
/* LOC_WINDOW_KERNEL_* of the node's last solve (LOC_WINDOW_KERNEL_NONE before the first) */
int loc_node_last_kernel_kind(const loc_node* n, int32_t* kind);
/* Localization::~Localization (localization.cpp:708-717): at destruction the reference appends path->poses[T/2 .. T-1] of the moving
 * tag to its "optimized" log (every earlier row of that log is a published path[T/2]), so that the log ends with the newest half of the
 * window.  Returns those rows (oldest first, 8 doubles each, the same poses loc_node_get_path gives at [T/2 .. T-1]) and their number;
 * LOC_ERR_INVALID when capacity_poses < T - T/2.  The node stays usable. */
int loc_node_flush_tail(loc_node* n, double* out_rows_by_8, int32_t capacity_poses);
/* Fleet mode: with deferred on, add_* only mark the node "solve pending"; loc_nodes_solve_batch then solves every
 * pending node of the array in ONE launch per parameter group (returns how many were solved). */
int loc_node_set_deferred(loc_node* n, int32_t on);
int32_t loc_node_solve_pending(const loc_node* n);
int loc_nodes_solve_batch(loc_node** nodes, int32_t n_nodes, loc_node_output* outs);
/* loc_nodes_solve_batch groups the pending nodes by (device, maximum_iteration, jacobian) — one launch per group, every
 * node solved with its own parameters — and keeps one batch solver per group cached for the calling thread; this frees them. */
int loc_nodes_release_batch_cache(void);

/* ================================================================================================
 * Batched fusion snapshot solver — BASELINE config 3 (8 anchors + IMU orientation prior, 6-DoF state).
 * Per tag and epoch, in the order the reference's callbacks produce it:
 *   IMU quaternion overwrites the rotation, translation kept                    localization.cpp:505-513
 *   EdgeSE3Prior on that pose, information diag(0,0,0,1/c0,1/c4,1/c8)            localization.cpp:515-525
 *   M EdgeSE3Range factors with the antenna lever arm on the tag side            localization.cpp:331-336
 *   outlier gate on the vertex origins, warm-up as in loc_snapshot_*             localization.cpp:306-313
 *   Localization::solve() on the 6-DoF vertex, optimizer.chi2()                  localization.cpp:164-170, 197
 * Device layouts:
 *   dist, err : float  [K][2][B][4]   as loc_snapshot_* with M <= 8
 *   imu       : double [K][B][8]      q x y z w, orientation_covariance[0], [4], [8], pad
 *   pose      : double [7][B]         state t xyz, q xyzw (in: initial, out: last); outputs [K][7][B], chi2 [K][B]
 * ============================================================================================== */
typedef struct loc_fusion loc_fusion;
typedef struct loc_fusion_params {
    int32_t maximum_iteration;   /* optimizer/maximum_iteration */
    double distance_outlier;     /* robot/distance_outlier; <= 0 disables */
    int32_t gate_warmup_epochs;  /* default 1 */
    double antenna_offset[3];    /* /uwb/antennaOffset of the antenna every range uses (localization.cpp:111-123, 333) */
    int32_t block_threads;       /* 0 = 256 */
    int32_t jacobian;            /* LOC_JAC_* for the range factors; default LOC_JAC_NUMERIC_G2O */
} loc_fusion_params;

void loc_fusion_default_params(loc_fusion_params* p);
int loc_fusion_create(loc_fusion** out, int32_t device, int64_t batch, int32_t n_anchors, const double* anchors_xyz_host,
                      const loc_fusion_params* params);
int loc_fusion_destroy(loc_fusion* f);
int loc_fusion_set_poses(loc_fusion* f, const double* pose_soa_host /* [7][B] */);
int loc_fusion_get_poses(loc_fusion* f, double* pose_soa_host);
int loc_fusion_solve_device(loc_fusion* f, int32_t epochs, const float* dist_dev, const float* err_dev, const double* imu_dev,
                            double* out_pose_dev, double* out_chi2_dev, uint8_t* out_trials_dev, void* hip_stream);
int loc_fusion_solve_host(loc_fusion* f, int32_t epochs, const float* dist_tiles_host, const float* err_tiles_host,
                          const double* imu_host, double* out_pose_host, double* out_chi2_host, uint8_t* out_trials_host);
/* Host arrays in their natural layout: dist/err [K][M][B] float32, imu [K][B][8]; tiles are packed on the GPU and the call
 * is pipelined like loc_snapshot_solve_host_kmb (page-locked buffers from loc_host_alloc overlap the copies). */
int loc_fusion_solve_host_kmb(loc_fusion* f, int32_t epochs, const float* dist_kmb_host, const float* err_kmb_host,
                              const double* imu_host, double* out_pose_host, double* out_chi2_host, uint8_t* out_trials_host);
/* Per-update marginal covariances of the 6-DoF pose, as loc_snapshot_solve_*_cov: H also holds the IMU prior's
 * term; coordinates are g2o VertexSE3's minimal increment [dt (body frame), dq_xyz] applied as X * fromVectorMQT(d).
 *   cov    double [K][21][B]  row-major upper triangle of the 6x6 Sigma in [tx ty tz qx qy qz]; NaN when singular
 *   mask   int32  [K][B]      bits 0-5 = tx ty tz qx qy qz excluded (an exactly zero diagonal entry of H)
 *   status int32  [K][B]      LOC_OK or LOC_ERR_SINGULAR */
int loc_fusion_solve_device_cov(loc_fusion* f, int32_t epochs, const float* dist_dev, const float* err_dev, const double* imu_dev,
                                double* out_pose_dev, double* out_chi2_dev, uint8_t* out_trials_dev,
                                double* out_cov_dev, int32_t* out_cov_mask_dev, int32_t* out_cov_status_dev, void* hip_stream);
int loc_fusion_solve_host_kmb_cov(loc_fusion* f, int32_t epochs, const float* dist_kmb_host, const float* err_kmb_host,
                                  const double* imu_host, double* out_pose_host, double* out_chi2_host, uint8_t* out_trials_host,
                                  double* out_cov_host, int32_t* out_cov_mask_host, int32_t* out_cov_status_host);
int loc_fusion_last_kernel_ms(loc_fusion* f, double* ms);
/* per-launch HIP-event pairs on the launch stream, as loc_snapshot_timing_* */
int loc_fusion_timing_begin(loc_fusion* f, int32_t max_launches);
int loc_fusion_timing_end(loc_fusion* f, int32_t* n_launches, double* total_ms, double* avg_ms);

#ifdef __cplusplus
}
#endif
#endif /* LOCALIZATION_AMD_H */
