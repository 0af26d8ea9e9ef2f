// C ABI of the batched sliding-window solver (see include/localization_amd.h). Host side only.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include <algorithm>
#include <chrono>
#include <new>
#include <string>
#include <vector>

#include "arrow_pack.h"
#include "capi_host.h"
#include "message_rows.h"
#include "slide_plain_admit.h"
#include "window_admit.h"
#include "window_dispatch.h"
#include "window_groups.h"
#include "window_kernel.h"
#include "window_layouts.h"
#include "window_structure.h"
#include "window_tables.h"

using locamd::kPoses;
using locamd::kCounts;
using locamd::CovKind;

// What the handle knows about the batch loc_window_upload left in the device arrays.  `Resident{}` is "none" (drop_resident): the resident
// calls return LOC_ERR_INVALID until the next upload completes, and nothing reads another field while n is 0.
struct Resident {
    long long n = 0;
    int topology = LOC_WINDOW_KERNEL_GENERAL;   // LOC_WINDOW_KERNEL_* the batch qualifies for by its structure (the batch-size threshold is applied per solve)
    bool skip = false;              // ... a verdict taken with the priors' diagonals skipped (a structured table was set): it holds while structured_pinfo(opt) does
    int min_anchors = 0;            // anchors the batch references (loc_window_set_anchors may not shrink below it)
    bool solved = false;            // a resident solve has run since the upload (loc_window_download has something to fetch)
    CovKind cov = CovKind::None;    // the batch's covariance pass; Unclassified: the first covariance call finds out
    bool groups_no_chain = false;   // loc_window_upload put the batch on the grouped solve path (slot[1].aux's groups block is on the device) and found no chain in any
                                    // edge order: under options "forest_groups" + "forest_groups_covariance" its covariance pass walks that block (resident_groups_covariance)
    long long env_switches = 0;     // cov_switches() when it was classified: a change of the switches the structured tests read classifies an Envelope batch again
    // joint covariance calls: the counts as uploaded (the pair check needs every window's nv) and, once the envelope pass holds the batch,
    // its pose-to-pose index tables (the pairs enlarge the envelope)
    std::vector<int32_t> counts, ridx, sidx;
    // the resident slide: with option "resident_slide" the upload keeps the batch's index tables next to counts (the mirror the slide's
    // admission counts from and slide_indices rewrites)
    bool mirror_valid = false, mirror_stale = false;   // stale: loc_window_slide_resident_dev has slid the device tables since the mirror was written (refresh_mirror)
    std::vector<int32_t> mir_ridx, mir_pidx;
};

struct loc_window {
    int device = 0;
    long long B = 0;
    locamd::WindowCaps caps{};
    int n_anchors = 0, anchors_cap = 0;
    int iterations = 10;
    int jacobian = LOC_JAC_NUMERIC_G2O;   // default = the reference's configuration (as is opt.natural_order = false)
    double* d_anchors = nullptr;
    std::vector<double> h_anchors;   // handles of <= 4 windows (a node's own): the table as last set; the device copy follows on demand
    bool anchors_dirty = false;
    locamd::DeviceTables dev{};     // the batch of the large host path, or the resident one ([kPoses]: the optimised estimates)
    double* d_result = nullptr;
    double* d_workspace = nullptr;  // HBM copy of the (H, L) matrices when they do not fit LDS
    double* d_poses_in = nullptr;   // resident mode: the uploaded initial estimates (every resident solve starts from them)
    double* d_chain_ws = nullptr;   // chain windows (one lane per window, chain_kernel.hip: chain_lm_kernel): its workspace
    double* d_chain3_ws = nullptr;  // translation-only chain windows (chain3_kernel.hip)
    // What belongs to ONE batch: slot[0] is the host path's (loc_window_solve_host, loc_window_covariance_host), slot[1] the resident batch's
    // from its upload on (a host-path call in between must not disturb it).
    struct BatchSlot {
        locamd::WinAux aux;       // the solve's host-built tables.  The host path's topology cache and the resident solve rely on them: no covariance call writes here
        // forest batches (forest_covariance_kernel.hip): the schedule — or, for windows of differing topologies, the groups block — the covariance
        // pass builds itself: slot[0]'s is kept with the hash of the structure it was built for (cov_sched), slot[1]'s is for a resident
        // batch no solve classified as a forest.
        // arrowhead batches (arrow_covariance_kernel.hip): cov_aux takes build_arrow_aux's structure test (never aux: the solve's packed tables stay as they are)
        locamd::WinAux cov_aux;
        double* d_cov_ws = nullptr;   // the arrowhead pass's HBM workspace (records, B, Y, the poses' edge lists), allocated on first use and grown on demand
        size_t cov_ws_cap = 0;        // doubles
        int cov_list_cap = 0;         // list size the batch was classified with
        // any other batch (envelope_covariance_kernel.hip, option "covariance_general"): the kernel's HBM workspace (the envelope of every window,
        // one column, diag(H)), grown on demand; the batch's largest envelope in blocks
        double* d_env_ws = nullptr;
        size_t env_ws_cap = 0;        // doubles
        long long env_blocks = 0;
    } slot[2];
    double* d_tree_ws = nullptr;    // workspaces (used only while a launch runs)
    double* d_arrow_ws = nullptr;
    size_t arrow_ws_nb = 0;         // border size d_arrow_ws was allocated for
    double* d_roff1 = nullptr;      // optional lever arms of endpoint 1 (loc_window_set_endpoint1_offsets: opt.has_off1), [B][nr_max][3]
    double* d_pinfo = nullptr;      // optional full information matrices of the priors (loc_window_set_prior_information: opt.has_pinfo), [B][np_max][36]
    long long n_pinfo = 0;          // instances the table describes: a call with more is refused
    Resident res;
    int last_kind = -1;             // LOC_WINDOW_KERNEL_* of the last launch
    int last_cov_kind = LOC_WINDOW_COV_NONE;   // loc_window_last_covariance_kind: the pass of the last covariance call that launched
    hipEvent_t resident_done = nullptr;  // recorded after every resident launch on the stream it ran on: whatever touches the shared
    bool resident_inflight = false;      // device state waits for THIS (the caller's stream is not kept: it may be destroyed any time)
    locamd::DispatchOpts opt;       // the kernel-selection switches (window_dispatch.h)
    locamd::DispatchFits fits;      // what the capacities alone decide, from loc_window_create
    locamd::TopoCache topo_cache;   // the host path's structural verdict
    double t_validate_ms = 0, t_topology_ms = 0, t_run_ms = 0;   // loc_window_last_host_timing
    int32_t last_groups = 0;        // loc_window_forest_groups: what the last structural verdict (host path or upload) found
    int64_t last_groups_bytes = 0;
    bool t_cached = false;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    double last_ms = 0.0;
    locamd::LaunchTimer timer;      // loc_window_timing_*: one pair per resident launch
    // small calls (a node's single window): all inputs travel as one page-locked block, all outputs as another
    char *h_stage = nullptr, *d_stage = nullptr;
    // marginal covariances (loc_window_covariance_*): a device block of their own for batches beyond the staging block, HIP events of
    // their own (the solve's last_kernel_ms stays as it is)
    char* d_cov = nullptr;
    size_t cov_cap = 0;
    hipEvent_t cov_ev0 = nullptr, cov_ev1 = nullptr;
    bool cov_pending = false;       // the events of a resident covariance launch have not been read yet
    double cov_ms = 0.0;
    locamd::SchedKey cov_sched;      // the structure slot[0].cov_aux's forest schedule was built (and uploaded) for
    // the call's host arrays on their way to the caller's stream: a resident joint call's pair tables [counts | pairs], a host slide's
    // inputs [drop | counts | new rows]
    locamd::StagingPair pairs, slide;
    bool opt_slide = false;         // option "resident_slide"
    char* d_slide_mp = nullptr;     // a slide's marginal pass: its drop table (zeros) and results for B windows (slide_marginal_layout)
    // rows from raw messages (loc_window_set_message_config): the configuration, the antenna table's device copy and the handle's own block of
    // window_message_kernel's outputs for B windows (message_rows_layout), which loc_window_push_messages_resident_dev builds into
    bool msg_set = false;
    loc_window_message_config msg_cfg{};
    int n_antenna = 0, antenna_cap = 0;
    double* d_antenna = nullptr;
    char* d_msg_rows = nullptr;
    // loc_window_upload_dev: the admit pass's device block [flags u64 [B] | kAdmitMaxWaves partial records | the record] and the record's page-locked copy
    char* d_admit = nullptr;
    locamd::WindowAdmitRecord* h_admit_record = nullptr;
    // ... under option "upload_dev_structures": the structure pass's device block [kStructMaxWaves partial records | the record] and the record's page-locked copy
    char* d_struct = nullptr;
    locamd::WindowStructRecord* h_struct_record = nullptr;
    // ... under option "upload_dev_forest_groups": the grouping pass's device block for B windows (dev_forest_groups lays it out), the record's
    // page-locked copy, and the compact tables of the representatives [counts | r_idx | p_idx | s_idx], grown to the groups of the batch
    char* d_groups_pass = nullptr;
    locamd::WindowGroupsRecord* h_groups_record = nullptr;
    int32_t* d_groups_compact = nullptr;
    size_t groups_compact_cap = 0;   // windows
};
static constexpr size_t kStageBytes = 4u << 20;
static constexpr size_t kResultBytes = 8 * sizeof(double);   // one instance's row of `result`

extern "C" {

static locamd::WindowCaps to_caps(const loc_window_caps* caps) {
    int bw = caps->bw_max < 0 ? caps->nv_max - 1 : caps->bw_max;
    if (bw > caps->nv_max - 1) bw = caps->nv_max - 1;
    if (bw < 0) bw = 0;
    return locamd::WindowCaps{caps->nv_max, caps->nr_max, caps->np_max, caps->ns_max, bw};
}

size_t loc_window_lds_bytes(const loc_window_caps* caps) {
    if (!caps) return 0;
    if (caps->nv_max <= 0) return 0;
    locamd::WindowCaps c = to_caps(caps);
    return locamd::window_arrays_in_lds(c) ? locamd::window_lds_bytes(c, false) : locamd::window_lds_bytes(c, true) + 36 * sizeof(double);  // large windows: index tables + exchange block; the rest in the HBM workspace
}

// every device buffer of one batch's slot
static void release_slot(loc_window::BatchSlot& S) {
    for (locamd::WinAux* A : {&S.aux, &S.cov_aux})
        for (void* p : {(void*)A->d_tsched, (void*)A->d_groups, (void*)A->d_ahdr, (void*)A->d_arslot, (void*)A->d_arec, (void*)A->d_aprec}) if (p) (void)hipFree(p);
    if (S.d_cov_ws) (void)hipFree(S.d_cov_ws);
    if (S.d_env_ws) (void)hipFree(S.d_env_ws);
}

int loc_window_destroy(loc_window* w) {
    if (!w) return LOC_OK;
    (void)hipSetDevice(w->device);
    void* ptrs[] = {w->d_anchors, w->d_result, w->d_workspace, w->d_poses_in, w->d_chain_ws, w->d_chain3_ws, w->d_roff1, w->d_pinfo, w->d_tree_ws, w->d_arrow_ws,
                    w->d_stage, w->d_cov, w->d_slide_mp, w->d_antenna, w->d_msg_rows, w->d_admit, w->d_struct, w->d_groups_pass, w->d_groups_compact};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    if (w->h_struct_record) (void)hipHostFree(w->h_struct_record);
    if (w->h_groups_record) (void)hipHostFree(w->h_groups_record);
    for (loc_window::BatchSlot& S : w->slot) release_slot(S);
    for (void* p : w->dev.t) if (p) (void)hipFree(p);
    if (w->h_stage) (void)hipHostFree(w->h_stage);
    if (w->h_admit_record) (void)hipHostFree(w->h_admit_record);
    w->timer.destroy(); w->pairs.destroy(); w->slide.destroy();
    for (hipEvent_t e : {w->ev0, w->ev1, w->resident_done, w->cov_ev0, w->cov_ev1}) if (e) (void)hipEventDestroy(e);
    if (w->stream) (void)hipStreamDestroy(w->stream);
    delete w;
    return LOC_OK;
}

int loc_window_create(loc_window** out, int32_t device, int64_t batch, const loc_window_caps* caps,
                      int32_t n_anchors, const double* anchors, int32_t maximum_iteration) {
    if (!out) return locamd_fail(LOC_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (batch <= 0 || !caps || n_anchors < 0 || (n_anchors > 0 && !anchors)) return locamd_fail(LOC_ERR_INVALID, "window arguments");
    if (caps->nv_max <= 0 || caps->nv_max > 4096 || caps->nr_max < 0 || caps->np_max < 0 || caps->ns_max < 0)
        return locamd_fail(LOC_ERR_UNSUPPORTED, "window capacities (1 <= nv_max <= 4096)");

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return locamd_fail(LOC_ERR_NO_DEVICE, "no HIP device visible: localization_amd has no CPU fallback");
    if (device < 0 || device >= ndev) return locamd_fail(LOC_ERR_INVALID, "device index out of range");
    LOC_HIP(hipSetDevice(device));
    loc_window* w = new (std::nothrow) loc_window();
    if (!w) return locamd_fail(LOC_ERR_INVALID, "out of host memory");
    w->device = device; w->B = batch; w->n_anchors = n_anchors; w->anchors_cap = n_anchors > 0 ? n_anchors : 1; w->iterations = maximum_iteration;
    w->caps = to_caps(caps);
    w->fits = locamd::dispatch_fits(w->caps);
    const bool global_a = !locamd::window_arrays_in_lds(w->caps);
    const size_t B = (size_t)batch;
    const size_t na = (size_t)(n_anchors > 0 ? n_anchors : 1);
    hipError_t e = hipSuccess;
    auto alloc = [&](void** p, size_t bytes) { return hipMalloc(p, bytes ? bytes : 8); };
    for (int t = 0; t < locamd::kWindowTables && e == hipSuccess; ++t) e = alloc(&w->dev.t[t], B * locamd::table_bytes(w->caps, t));
    if (e != hipSuccess || (e = alloc((void**)&w->d_anchors, na * 3 * sizeof(double))) != hipSuccess ||
        // (the solve kernels write the pose slots a window uses: what lies behind a window's nv in the output array reads as 0 after a
        //  download, on every handle alike, not as whatever a recycled allocation held)
        (e = hipMemset(w->dev.t[kPoses], 0, B * locamd::table_bytes(w->caps, kPoses))) != hipSuccess ||
        (e = alloc((void**)&w->d_result, B * kResultBytes)) != hipSuccess ||
        (global_a && (e = hipMalloc((void**)&w->d_workspace, B * locamd::window_workspace_doubles(w->caps) * sizeof(double))) != hipSuccess) ||
        (e = hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipEventCreate(&w->ev0)) != hipSuccess || (e = hipEventCreate(&w->ev1)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&w->resident_done, hipEventDisableTiming)) != hipSuccess ||
        (e = hipEventCreate(&w->cov_ev0)) != hipSuccess || (e = hipEventCreate(&w->cov_ev1)) != hipSuccess ||
        (n_anchors > 0 && (e = hipMemcpy(w->d_anchors, anchors, (size_t)n_anchors * 3 * sizeof(double), hipMemcpyHostToDevice)) != hipSuccess)) {
        loc_window_destroy(w);
        return locamd_fail_hip(e, "loc_window_create");
    }
    if (batch <= 4 && n_anchors > 0) w->h_anchors.assign(anchors, anchors + (size_t)n_anchors * 3);
    {   // the A/B switches of the environment, read once
        locamd::DispatchOpts& o = w->opt;
        if (const char* v = getenv("LOCAMD_CHAIN_MIN_BATCH")) { o.env_chain_min = atoll(v); o.env_chain_min_set = true; }
        if (const char* v = getenv("LOCAMD_ARROW3")) o.arrow3 = v[0] == '1' ? 1 : 0;
        if (const char* v = getenv("LOCAMD_TREE")) o.tree = v[0] == '0' ? 0 : (v[0] == 'l' ? 2 : -1);
        if (const char* v = getenv("LOCAMD_WAVE3")) o.wave3 = v[0] != '0';
        if (const char* v = getenv("LOCAMD_WAVE6")) o.wave6 = v[0] != '0';
        if (const char* v = getenv("LOCAMD_CHAIN3")) o.chain3 = v[0] != '0';
        if (getenv("LOCAMD_NO_ZERO_COPY")) o.zero_copy = false;
        if (const char* v = getenv("LOCAMD_KERNEL_EVENTS")) o.kernel_events = atoi(v) != 0;
    }
    *out = w;
    return LOC_OK;
}

// n instances of every table with bytes and a destination from src to dst: hipMemcpyAsync on *stream, or hipMemcpy where it is nullptr
static hipError_t copy_tables(const locamd::WindowCaps& c, size_t n, void* const* dst, const void* const* src, hipMemcpyKind kind, const hipStream_t* stream) {
    for (int t = 0; t < locamd::kWindowTables; ++t) {
        const size_t bytes = n * locamd::table_bytes(c, t);
        if (!bytes || !dst[t]) continue;
        const hipError_t e = stream ? hipMemcpyAsync(dst[t], src[t], bytes, kind, *stream) : hipMemcpy(dst[t], src[t], bytes, kind);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// whatever is about to touch the device state a resident launch reads or writes waits for that launch first
static int wait_resident(loc_window* w) {
    if (!w->resident_inflight) return LOC_OK;
    LOC_HIP(hipEventSynchronize(w->resident_done));
    w->resident_inflight = false;
    return LOC_OK;
}

// After loc_window_slide_resident_dev — and after loc_window_upload_dev, which copies no integer table to the host — the device holds the only
// copy of the counts and index tables.  Whoever reads the host's copies (res.counts, res.mir_ridx, res.mir_pidx, res.min_anchors) asks here
// first: waits for the resident work, fetches counts and, where the batch has a mirror (option "resident_slide" at its upload), r_idx and p_idx,
// and recomputes the largest anchor referenced from them.  A batch without a mirror fetches counts alone: only loc_window_upload_dev leaves such
// a batch stale, and its min_anchors came from the admit pass's record.  Nothing to do (and no wait) while the copies are current.
static int refresh_mirror(loc_window* w) {
    Resident& R = w->res;
    if (!R.mirror_stale) return LOC_OK;
    LOC_HIP(hipSetDevice(w->device));
    if (int rc = wait_resident(w)) return rc;
    const locamd::WindowCaps& c = w->caps;
    const size_t N = (size_t)R.n;
    LOC_HIP(hipMemcpy(R.counts.data(), w->dev.t[kCounts], N * 4 * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (R.mirror_valid) {
        if (c.nr_max) LOC_HIP(hipMemcpy(R.mir_ridx.data(), w->dev.t[locamd::kRIdx], N * c.nr_max * 2 * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (c.np_max) LOC_HIP(hipMemcpy(R.mir_pidx.data(), w->dev.t[locamd::kPIdx], N * c.np_max * sizeof(int32_t), hipMemcpyDeviceToHost));
        R.min_anchors = locamd::max_anchor_referenced(c, R.n, R.counts.data(), R.mir_ridx.data());
    }
    R.mirror_stale = false;
    return LOC_OK;
}

// the device copy of the anchor table
static int upload_anchors(loc_window* w, int32_t n_anchors, const double* anchors) {
    LOC_HIP(hipSetDevice(w->device));
    if (int rc = wait_resident(w)) return rc;   // a resident launch may still be reading the table
    if (n_anchors > w->anchors_cap) {
        double* p = nullptr;
        LOC_HIP(hipMalloc((void**)&p, (size_t)n_anchors * 3 * sizeof(double)));
        if (w->d_anchors) (void)hipFree(w->d_anchors);
        w->d_anchors = p;
        w->anchors_cap = n_anchors;
    }
    if (n_anchors > 0) LOC_HIP(hipMemcpy(w->d_anchors, anchors, (size_t)n_anchors * 3 * sizeof(double), hipMemcpyHostToDevice));
    w->n_anchors = n_anchors;
    w->anchors_dirty = false;
    return LOC_OK;
}
static int flush_anchors(loc_window* w) {
    if (!w->anchors_dirty) return LOC_OK;
    return upload_anchors(w, w->n_anchors, w->h_anchors.data());
}

int loc_window_set_anchors(loc_window* w, int32_t n_anchors, const double* anchors) {
    if (!w || n_anchors < 0 || (n_anchors > 0 && !anchors)) return locamd_fail(LOC_ERR_INVALID, "set_anchors");
    if (int rc = refresh_mirror(w)) return rc;   // (a slide from device arrays may have introduced anchors the host has not seen)
    if (w->res.n > 0 && n_anchors < w->res.min_anchors)
        return locamd_fail(LOC_ERR_INVALID, "set_anchors: the resident batch references more anchors than the new table holds (upload again first)");
    if (w->B <= 4) {
        // a node's handle: its table changes with every message (the window slides), and its solve usually reads the table from the
        // page-locked staging block (loc_window_solve_host) — the device copy is refreshed only when a launch needs it
        w->h_anchors.assign(anchors, anchors + (size_t)n_anchors * 3);
        w->n_anchors = n_anchors;
        w->anchors_dirty = true;
        return LOC_OK;
    }
    return upload_anchors(w, n_anchors, anchors);
}

// the checks of a batch's arguments that read no table (b's pointers are looked at, never followed: host or device arrays alike)
static int validate_arguments(const loc_window* w, const locamd::HostBatch& b) {
    if (!w || !b.counts || !b.poses) return locamd_fail(LOC_ERR_INVALID, "window solve arguments");
    if (b.n <= 0 || b.n > w->B) return locamd_fail(LOC_ERR_INVALID, "n_instances");
    if (w->opt.has_pinfo && b.n > w->n_pinfo) return locamd_fail(LOC_ERR_INVALID, "n_instances: more windows than loc_window_set_prior_information described");
    const locamd::WindowCaps& c = w->caps;
    if ((c.nr_max && (!b.r_idx || !b.r_val)) || (c.np_max && (!b.p_idx || !b.p_val)) || (c.ns_max && (!b.s_idx || !b.s_val)))
        return locamd_fail(LOC_ERR_INVALID, "missing edge arrays");
    return LOC_OK;
}
// the words of check_instances' / window_admit.h's codes
static const char* const kInstanceCheck[] = {nullptr, "counts exceed capacities", "range edge vertex index", "range edge couples poses further apart than bw_max",
                                             "prior edge vertex index", "SE3 edge vertex index", "SE3 edge couples poses further apart than bw_max"};
// host-side shape check: a bad index would fault the GPU
static int validate_instances(const loc_window* w, const locamd::HostBatch& b) {
    if (int rc = validate_arguments(w, b)) return rc;
    if (const int bad = locamd::check_instances(w->caps, w->n_anchors, b)) return locamd_fail(LOC_ERR_INVALID, kInstanceCheck[bad]);
    return LOC_OK;
}

// the device tables of arrow3_lm_kernel for B windows: hdr and rslot
static hipError_t reserve_arrow_rows(loc_window* w, locamd::WinAux& A) {
    if (A.d_ahdr) return hipSuccess;
    const hipError_t e = hipMalloc((void**)&A.d_ahdr, (size_t)w->B * 8 * sizeof(int32_t));
    return e != hipSuccess ? e : hipMalloc((void**)&A.d_arslot, (size_t)w->B * w->caps.nv_max * sizeof(int32_t));
}
// ... the record tables for n windows of rec_used / prec_used doubles in all, and the kernel's workspace for a border of A.arrow_nb_max
static hipError_t reserve_arrow_records(loc_window* w, locamd::WinAux& A, int64_t n, size_t rec_used, size_t prec_used) {
    const size_t B = (size_t)w->B, N = (size_t)n;
    // a record table that this batch's records outgrow is replaced by one for B windows of this batch's records per window
    auto grow_records = [&](double*& d, size_t& cap, size_t used) {
        if (used <= cap) return hipSuccess;
        cap = 0;
        return locamd::grow_buffers(cap, used / N * B, {{d, used / N * B * sizeof(double)}});
    };
    hipError_t e;
    if ((e = grow_records(A.d_arec, A.arec_cap, rec_used)) != hipSuccess || (e = grow_records(A.d_aprec, A.aprec_cap, prec_used)) != hipSuccess) return e;
    return locamd::grow_buffers(w->arrow_ws_nb, (size_t)A.arrow_nb_max,
                                {{w->d_arrow_ws, B * locamd::window_arrow3_workspace_doubles(w->caps, A.arrow_nb_max) * sizeof(double)}});
}

static hipError_t upload_arrow_aux(loc_window* w, loc_window::BatchSlot& S, int64_t n, hipStream_t st) {
    locamd::WinAux& A = S.aux;
    const locamd::WindowCaps& c = w->caps;
    const size_t N = (size_t)n;
    hipError_t e;
    if ((e = reserve_arrow_rows(w, A)) != hipSuccess || (e = reserve_arrow_records(w, A, n, A.h_arec.size(), A.h_aprec.size())) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(A.d_ahdr, A.h_ahdr.data(), N * 8 * sizeof(int32_t), hipMemcpyHostToDevice, st)) != hipSuccess ||
        (e = hipMemcpyAsync(A.d_arslot, A.h_arslot.data(), N * c.nv_max * sizeof(int32_t), hipMemcpyHostToDevice, st)) != hipSuccess ||
        (e = hipMemcpyAsync(A.d_arec, A.h_arec.data(), A.h_arec.size() * sizeof(double), hipMemcpyHostToDevice, st)) != hipSuccess ||
        (e = hipMemcpyAsync(A.d_aprec, A.h_aprec.data(), A.h_aprec.size() * sizeof(double), hipMemcpyHostToDevice, st)) != hipSuccess) return e;
    return hipStreamSynchronize(st);   // (the host vectors may be rebuilt by the next call)
}

// solve: the schedule is for a solve kernel (tree_lm_kernel's workspace is allocated); the covariance pass needs the tables alone
// groups: the batch is on the grouped path (LOC_WINDOW_KERNEL_TREE_GROUPS) — the block [hdr | sched_of | pad | tables] of build_tree_groups
// goes instead, into a buffer of its own (the one-topology table of the same slot stays as it is)
static hipError_t upload_tree_sched(loc_window* w, locamd::WinAux& A, hipStream_t st, bool solve = true, bool groups = false) {
    hipError_t e;
    if (groups) {
        if ((e = locamd::grow_buffers(A.groups_cap, A.h_groups.size(), {{A.d_groups, A.h_groups.size() * sizeof(int32_t)}})) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(A.d_groups, A.h_groups.data(), A.h_groups.size() * sizeof(int32_t), hipMemcpyHostToDevice, st)) != hipSuccess) return e;
        return hipStreamSynchronize(st);
    }
    if ((e = locamd::grow_buffers(A.tsched_cap, A.h_tsched.size(), {{A.d_tsched, A.h_tsched.size() * sizeof(int32_t)}})) != hipSuccess) return e;
    if (solve && !w->d_tree_ws && (e = hipMalloc((void**)&w->d_tree_ws, locamd::window_tree_workspace_doubles(w->caps, w->B) * sizeof(double))) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(A.d_tsched, A.h_tsched.data(), A.h_tsched.size() * sizeof(int32_t), hipMemcpyHostToDevice, st)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
    locamd::bind_tree_sched(A.tsched, A.d_tsched);
    return hipSuccess;
}

// the envelope pass's workspace for n windows of at most `blocks` envelope blocks
static hipError_t grow_env_workspace(loc_window* w, loc_window::BatchSlot& S, int64_t n, long long blocks) {
    const size_t need = (size_t)n * locamd::window_envelope_covariance_workspace_doubles(w->caps, blocks);
    return locamd::grow_buffers(S.env_ws_cap, need, {{S.d_env_ws, need * sizeof(double)}});
}
// the arrowhead pass's workspace for n windows with lists of `cap` entries
static hipError_t grow_cov_workspace(loc_window* w, loc_window::BatchSlot& S, int64_t n, int cap) {
    const size_t need = (size_t)n * locamd::window_arrow_covariance_workspace_doubles(w->caps, cap);
    return locamd::grow_buffers(S.cov_ws_cap, need, {{S.d_cov_ws, need * sizeof(double)}});
}

// the page-locked staging block of the small calls and its device twin
static int ensure_stage(loc_window* w) {
    if (!w->h_stage) LOC_HIP(hipHostMalloc((void**)&w->h_stage, kStageBytes, hipHostMallocDefault));
    if (!w->d_stage) LOC_HIP(hipMalloc((void**)&w->d_stage, kStageBytes));
    return LOC_OK;
}

// The kernels' arguments for n instances of the tables d.  poses_in: nullptr = d's own poses (solved in place; the resident solve starts
// from the uploaded ones).  anchors: w->d_anchors, or the zero-copy solve's copy behind the staging block.  result: nullptr = a covariance
// pass, which takes no lever arms of endpoint 1 and no workspace either.
static locamd::WindowArgs window_args(const loc_window* w, const locamd::DeviceTables& d, int64_t n, const double* poses_in, const double* anchors, double* result) {
    locamd::WindowArgs a;
    a.counts = (const int32_t*)d.t[kCounts]; a.poses = (double*)d.t[kPoses]; a.poses_in = poses_in ? poses_in : a.poses;
    a.r_idx = (const int32_t*)d.t[locamd::kRIdx]; a.r_val = (const double*)d.t[locamd::kRVal];
    a.p_idx = (const int32_t*)d.t[locamd::kPIdx]; a.p_val = (const double*)d.t[locamd::kPVal];
    a.s_idx = (const int32_t*)d.t[locamd::kSIdx]; a.s_val = (const double*)d.t[locamd::kSVal];
    a.anchors = anchors; a.result = result; a.r_off1 = result && w->opt.has_off1 ? w->d_roff1 : nullptr; a.p_info = w->opt.has_pinfo ? w->d_pinfo : nullptr; a.workspace = result ? w->d_workspace : nullptr;
    a.n_anchors = w->n_anchors; a.B = (int)n; a.iterations = w->iterations; a.jacobian = w->jacobian; a.natural_order = w->opt.natural_order; a.caps = w->caps;
    return a;
}
// the resident batch as uploaded: the initial estimates in the place of the optimised ones
static locamd::DeviceTables uploaded_tables(const loc_window* w) { locamd::DeviceTables d = w->dev; d.t[kPoses] = w->d_poses_in; return d; }
// the device arrays hold no resident batch any more (the resident calls return LOC_ERR_INVALID until the next loc_window_upload completes)
static void drop_resident(loc_window* w) { w->res = Resident{}; }
// The resident batch's structural verdict as it holds NOW.  One taken with the priors' diagonals skipped is worth nothing once the structured
// table has gone, has got rotation entries or the option is off — the diagonals in p_val count again and may hold rotation information: such a
// batch takes the general kernel until the next upload, never wave3_lm_kernel, and does not slide
static int resident_topology(const loc_window* w) { return w->res.skip && !locamd::structured_pinfo(w->opt) ? (int)LOC_WINDOW_KERNEL_GENERAL : w->res.topology; }

// What a resident entry refuses without looking at a window: the rule and its words are window_dispatch.cpp's resident_refusal.  The entry's own
// argument checks travel as arg_failed (0, or the first of them that fails, counted from 1): the rule knows their place between the state
// checks, and their words.  Nothing is launched or changed on a refusal
static int resident_gate(const loc_window* w, locamd::ResidentEntry e, int arg_failed = 0) {
    locamd::ResidentFacts f;
    if (w) {
        f.handle = true; f.resident = w->res.n > 0; f.mirror_valid = w->res.mirror_valid; f.solved = w->res.solved;
        f.pinfo_short = w->opt.has_pinfo && w->res.n > w->n_pinfo; f.topology = resident_topology(w);
        f.has_off1 = w->opt.has_off1; f.has_pinfo = w->opt.has_pinfo; f.pinfo_translation = w->opt.pinfo_translation; f.msg_set = w->msg_set;
    }
    const locamd::Refusal r = locamd::resident_refusal(e, f, arg_failed);
    return r.code == LOC_OK ? (int)LOC_OK : locamd_fail(r.code, r.text);
}

// ---- the launch bracket of the resident entries: the whole stream-ordering contract of the resident batch -------------------------------------
// First half: the device, the anchor table's device copy where the launch reads it (flush), the stream of the call.
static int resident_stream(loc_window* w, void* hip_stream, bool flush, hipStream_t& st) {
    LOC_HIP(hipSetDevice(w->device));
    if (flush)
        if (int rc = flush_anchors(w)) return rc;
    st = hip_stream ? (hipStream_t)hip_stream : w->stream;
    return LOC_OK;
}
// Second half: st waits for the last resident launch (it may have run on another stream), `staged` queues what the launch reads (outside the
// timing), `launch` runs between the timing's two records, and resident_done is recorded for whatever touches the resident arrays next —
// the next resident launch on any stream, wait_resident on the host.  Both callables return a LOC_* code.
enum class Timing { None, Solve, Covariance };   // none; loc_window_timing_*'s pair; cov_ev0 / cov_ev1 for loc_window_last_covariance_ms
extern "C++" {   // (a template cannot have C linkage)
template <class Staged, class Launch>
static int resident_bracket(loc_window* w, hipStream_t st, Timing timing, Staged&& staged, Launch&& launch) {
    if (w->resident_inflight) LOC_HIP(hipStreamWaitEvent(st, w->resident_done, 0));
    if (int rc = staged(st)) return rc;
    if (timing == Timing::Solve) LOC_HIP(w->timer.start(st));
    if (timing == Timing::Covariance) LOC_HIP(hipEventRecord(w->cov_ev0, st));
    if (int rc = launch(st)) return rc;
    if (timing == Timing::Solve) LOC_HIP(w->timer.stop(st));
    if (timing == Timing::Covariance) LOC_HIP(hipEventRecord(w->cov_ev1, st));
    LOC_HIP(hipEventRecord(w->resident_done, st));
    w->resident_inflight = true;
    if (timing == Timing::Covariance) w->cov_pending = true;
    return LOC_OK;
}
static int nothing_staged(hipStream_t) { return LOC_OK; }
// both halves, for an entry with no work of its own in between
template <class Launch>
static int resident_launch(loc_window* w, void* hip_stream, Timing timing, bool flush, Launch&& launch) {
    hipStream_t st;
    if (int rc = resident_stream(w, hip_stream, flush, st)) return rc;
    return resident_bracket(w, st, timing, nothing_staged, launch);
}
}   // extern "C++"
// a launcher's hipError_t as a LOC_* code
static int launched(hipError_t e, const char* what) { return e == hipSuccess ? (int)LOC_OK : locamd_fail_hip(e, what); }

static hipError_t launch_any(loc_window* w, loc_window::BatchSlot& S, const locamd::WindowArgs& a, hipStream_t st, int kind) {
    locamd::WinAux& A = S.aux;
    w->last_kind = kind;
    if (kind == LOC_WINDOW_KERNEL_ARROW3) {
        locamd::ArrowAux x;
        x.hdr = A.d_ahdr; x.rslot = A.d_arslot; x.rec = A.d_arec; x.prec = A.d_aprec;
        x.ws = w->d_arrow_ws; x.nb_max = A.arrow_nb_max; x.jmax = A.arrow_jmax; x.jpmax = A.arrow_jpmax; x.nchunk = (w->caps.nv_max + 63) / 64;
        for (int k = 0; k < 16; ++k) { x.jch[k] = A.arrow_jch[k]; x.jpch[k] = A.arrow_jpch[k]; }
        return locamd::launch_window_arrow3(a, x, st);
    }
    if (kind == LOC_WINDOW_KERNEL_TREE) {   // (option "tree" = 2: the one-lane-per-window variant, for A/B runs)
        if (w->opt.tree == 2 || A.tsched.max_se3_per_node > 1) {   // (tree_wave_kernel: one EdgeSE3 per node)
            w->last_kind = LOC_WINDOW_KERNEL_TREE_LANE;
            return locamd::launch_window_tree(a, A.tsched, w->d_tree_ws, st);
        }
        return locamd::launch_window_tree_wave(a, A.tsched, st);
    }
    if (kind == LOC_WINDOW_KERNEL_TREE_GROUPS) {
        if (A.n_groups <= 0 || !A.d_groups) return hipErrorInvalidValue;
        const locamd::TreeGroups g{A.d_groups, A.d_groups + A.groups_of_at, A.d_groups + A.groups_tab_at, A.n_groups};
        return locamd::launch_window_tree_wave_groups(a, g, A.h_groups.data(), st);
    }
    if (kind == LOC_WINDOW_KERNEL_CHAIN3) {
        if (!w->d_chain3_ws) {
            hipError_t e = hipMalloc((void**)&w->d_chain3_ws, locamd::window_chain3_workspace_doubles(w->caps, w->B) * sizeof(double));
            if (e != hipSuccess) return e;
        }
        return locamd::launch_window_chain3(a, w->d_chain3_ws, st);
    }
    if (kind == LOC_WINDOW_KERNEL_WAVE3) return locamd::launch_window_wave3(a, st);
    if (kind == LOC_WINDOW_KERNEL_WAVE6) return locamd::launch_window_wave6(a, false, st);
    if (kind == LOC_WINDOW_KERNEL_WAVE6S) return locamd::launch_window_wave6(a, true, st);
    if (kind == LOC_WINDOW_KERNEL_GENERAL) return locamd::launch_window(a, st);
    if (!w->d_chain_ws) {
        hipError_t e = hipMalloc((void**)&w->d_chain_ws, locamd::window_chain_workspace_doubles(w->caps, w->B) * sizeof(double));
        if (e != hipSuccess) return e;
    }
    return locamd::launch_window_chain(a, w->d_chain_ws, st);
}

int loc_window_last_kernel_kind(const loc_window* w, int32_t* kind) {
    if (!w || !kind) return locamd_fail(LOC_ERR_INVALID, "null");
    *kind = w->last_kind;
    return LOC_OK;
}

int loc_window_set_chain_threshold(loc_window* w, int64_t min_batch) {
    if (!w) return locamd_fail(LOC_ERR_INVALID, "null");
    w->opt.chain_min = min_batch;
    return LOC_OK;
}

int loc_window_set_option(loc_window* w, const char* name, int64_t value) {
    if (!w || !name) return locamd_fail(LOC_ERR_INVALID, "set_option");
    const std::string k(name);
    locamd::DispatchOpts& o = w->opt;
    auto flag = [&](bool& f) { if (value != 0 && value != 1) return locamd_fail(LOC_ERR_INVALID, "set_option: 0 or 1"); f = value == 1; return (int)LOC_OK; };
    if (k == "chain_min_batch") { o.chain_min = value; return LOC_OK; }
    if (k == "arrow3") { if (value < -1 || value > 1) return locamd_fail(LOC_ERR_INVALID, "set_option arrow3: -1, 0 or 1"); o.arrow3 = (int)value; w->topo_cache.valid = false; return LOC_OK; }
    if (k == "tree") { if (value != -1 && value != 0 && value != 2) return locamd_fail(LOC_ERR_INVALID, "set_option tree: -1, 0 or 2"); o.tree = (int)value; w->topo_cache.valid = false; return LOC_OK; }
    if (k == "forest_groups") {   // (read by the structure test: loc_window_solve_host, loc_window_upload)
        w->topo_cache.valid = false;
        const bool before = o.forest_groups;
        const int rc = flag(o.forest_groups);
        // (with "forest_groups_covariance" 1 it is one of the two switches of the grouped covariance pass: a resident batch that was refused is classified again)
        if (rc == LOC_OK && before != o.forest_groups && o.forest_groups_cov && w->res.n > 0 && w->res.cov == CovKind::None) w->res.cov = CovKind::Unclassified;
        return rc;
    }
    if (k == "forest_groups_covariance") {
        const bool before = o.forest_groups_cov;
        const int rc = flag(o.forest_groups_cov);
        // as "covariance_general": a resident batch the other value refused, or left to the envelope pass, is classified again by the next covariance call
        if (rc == LOC_OK && before != o.forest_groups_cov && w->res.n > 0 && (w->res.cov == CovKind::None || w->res.cov == CovKind::Envelope)) w->res.cov = CovKind::Unclassified;
        return rc;
    }
    if (k == "wave3") return flag(o.wave3);
    if (k == "wave6") return flag(o.wave6);
    if (k == "chain3") return flag(o.chain3);
    if (k == "zero_copy") return flag(o.zero_copy);
    if (k == "kernel_events") return flag(o.kernel_events);
    if (k == "covariance_general") {
        const bool before = o.cov_general;
        const int rc = flag(o.cov_general);
        // a resident batch the other value refused, or handed to the envelope pass, is classified again by the next covariance call
        if (rc == LOC_OK && before != o.cov_general && w->res.n > 0 && (w->res.cov == CovKind::None || w->res.cov == CovKind::Envelope)) w->res.cov = CovKind::Unclassified;
        return rc;
    }
    if (k == "prior_information_structured") {
        const bool before = o.pinfo_structured;
        const int rc = flag(o.pinfo_structured);
        // a resident batch under a table is classified again by the next covariance call: the other value takes another pass (or none)
        if (rc == LOC_OK && before != o.pinfo_structured && w->res.n > 0 && o.has_pinfo) w->res.cov = CovKind::Unclassified;
        return rc;
    }
    if (k == "resident_slide") return flag(w->opt_slide);   // (read by loc_window_upload: the batch resident now keeps what its upload decided)
    if (k == "topology_cache") { w->topo_cache.valid = false; return flag(o.topology_cache); }
    if (k == "upload_dev_structures") return flag(o.upload_dev_structures);   // (read by loc_window_upload_dev: the batch resident now keeps what its upload decided)
    if (k == "upload_dev_forest_groups") return flag(o.upload_dev_forest_groups);   // (likewise)
    if (k == "upload_dev_groups_hash_bits") {   // (a test seam: the device's candidate hash keeps this many low bits)
        if (value < 0 || value > 64) return locamd_fail(LOC_ERR_INVALID, "set_option upload_dev_groups_hash_bits: 0 .. 64");
        o.upload_dev_groups_hash_bits = (int)value;
        return LOC_OK;
    }
    return locamd_fail(LOC_ERR_INVALID, "set_option: unknown option name");
}

int loc_window_last_host_timing(const loc_window* w, double* out) {
    if (!w || !out) return locamd_fail(LOC_ERR_INVALID, "null");
    out[0] = w->t_validate_ms; out[1] = w->t_topology_ms; out[2] = w->t_run_ms; out[3] = w->t_cached ? 1.0 : 0.0;
    return LOC_OK;
}

int loc_window_forest_groups(const loc_window* w, int32_t* n_groups, int64_t* table_bytes) {
    if (!w || !n_groups || !table_bytes) return locamd_fail(LOC_ERR_INVALID, "null");
    *n_groups = w->last_groups; *table_bytes = w->last_groups_bytes;
    return LOC_OK;
}

int loc_window_set_endpoint1_offsets(loc_window* w, int64_t n, const double* off1) {
    if (!w || (off1 && (n <= 0 || n > w->B))) return locamd_fail(LOC_ERR_INVALID, "set_endpoint1_offsets");
    if (!off1) { w->opt.has_off1 = false; return LOC_OK; }   // (has_off1 is part of the structure hash: no cache entry survives a change of it)
    if (w->caps.nr_max <= 0) return locamd_fail(LOC_ERR_INVALID, "set_endpoint1_offsets: no range edges in this solver");
    LOC_HIP(hipSetDevice(w->device));
    if (int rc = wait_resident(w)) return rc;
    LOC_HIP(hipStreamSynchronize(w->stream));
    const size_t row = (size_t)w->caps.nr_max * 3 * sizeof(double);
    if (!w->d_roff1) LOC_HIP(hipMalloc((void**)&w->d_roff1, (size_t)w->B * row));
    LOC_HIP(hipMemcpy(w->d_roff1, off1, (size_t)n * row, hipMemcpyHostToDevice));
    // rows [n, B): no lever arm (a call with fewer instances than an earlier one must not leave that one's behind)
    if (n < w->B) LOC_HIP(hipMemset((char*)w->d_roff1 + (size_t)n * row, 0, (size_t)(w->B - n) * row));
    w->opt.has_off1 = true;
    return LOC_OK;
}

int loc_window_set_prior_information(loc_window* w, int64_t n, const double* pinfo) {
    if (!w) return locamd_fail(LOC_ERR_INVALID, "set_prior_information");
    // (option "prior_information_structured": the resident batch's covariance verdict may rest on the table that goes or changes here — the
    //  next covariance call classifies the batch again; its solve verdict is checked per solve, loc_window_solve_resident)
    if (w->opt.pinfo_structured && w->res.n > 0) w->res.cov = CovKind::Unclassified;
    if (!pinfo) { w->opt.has_pinfo = false; w->opt.pinfo_translation = false; w->n_pinfo = 0; return LOC_OK; }   // (has_pinfo is part of the structure hash, as has_off1 is)
    if (n <= 0 || n > w->B) return locamd_fail(LOC_ERR_INVALID, "set_prior_information: n_instances");
    if (w->caps.np_max <= 0) return locamd_fail(LOC_ERR_INVALID, "set_prior_information: no prior edges in this solver");
    // everything is checked before anything changes: a matrix that is not exactly symmetric (a NaN entry included) leaves the handle as it was
    const size_t rows = (size_t)n * w->caps.np_max;
    for (size_t e = 0; e < rows; ++e) {
        const double* W = pinfo + e * 36;
        for (int i = 1; i < 6; ++i)
            for (int j = 0; j < i; ++j)
                if (!(W[i * 6 + j] == W[j * 6 + i])) return locamd_fail(LOC_ERR_INVALID, "set_prior_information: an information matrix is not symmetric");
    }
    LOC_HIP(hipSetDevice(w->device));
    if (int rc = wait_resident(w)) return rc;
    LOC_HIP(hipStreamSynchronize(w->stream));
    const size_t row = (size_t)w->caps.np_max * 36 * sizeof(double);
    if (!w->d_pinfo) LOC_HIP(hipMalloc((void**)&w->d_pinfo, (size_t)w->B * row));
    LOC_HIP(hipMemcpy(w->d_pinfo, pinfo, (size_t)n * row, hipMemcpyHostToDevice));
    w->opt.has_pinfo = true;
    w->n_pinfo = n;
    w->opt.pinfo_translation = locamd::prior_information_translation_only(rows, pinfo);
    return LOC_OK;
}

int loc_window_set_jacobian(loc_window* w, int32_t jacobian) {
    if (!w || (jacobian != LOC_JAC_ANALYTIC && jacobian != LOC_JAC_NUMERIC_G2O)) return locamd_fail(LOC_ERR_INVALID, "jacobian mode");
    w->jacobian = jacobian;
    return LOC_OK;
}
int loc_window_set_ordering(loc_window* w, int32_t natural) {
    if (!w) return locamd_fail(LOC_ERR_INVALID, "null");
    w->opt.natural_order = natural != 0;
    return LOC_OK;
}

// loc_window_forest_groups: a structural verdict's groups (none unless it is the grouped path's)
static void note_groups(loc_window* w, const locamd::WinAux& A, int topology) {
    const bool on = topology == LOC_WINDOW_KERNEL_TREE_GROUPS;
    w->last_groups = on ? A.n_groups : 0;
    w->last_groups_bytes = on ? (int64_t)(A.h_groups.size() * sizeof(int32_t)) : 0;
}

// the kernel of a host-path batch: its structure (slot[0]'s tables, the topology cache), then the rules of the moment
static int host_kernel(loc_window* w, const locamd::HostBatch& b) {
    const locamd::Topology t = locamd::batch_topology(w->caps, w->opt, w->fits, w->n_anchors, b, w->slot[0].aux, &w->topo_cache);
    w->t_cached = t.cached;
    note_groups(w, w->slot[0].aux, t.kind);
    return locamd::pick_kernel(w->opt, w->fits, b.n, t.kind);
}

int loc_window_solve_host(loc_window* w, int64_t n, const int32_t* counts, double* poses, const int32_t* r_idx,
                          const double* r_val, const int32_t* p_idx, const double* p_val, const int32_t* s_idx,
                          const double* s_val, double* result) {
    if (!result) return locamd_fail(LOC_ERR_INVALID, "window solve arguments");
    using clk = std::chrono::steady_clock;
    auto ms_since = [](clk::time_point t) { return std::chrono::duration<double, std::milli>(clk::now() - t).count(); };
    const auto t_begin = clk::now();
    const locamd::HostBatch b{n, poses, counts, r_val, p_val, s_val, r_idx, p_idx, s_idx};
    if (int rc = validate_instances(w, b)) return rc;
    w->t_validate_ms = ms_since(t_begin);
    const locamd::WindowCaps& c = w->caps;
    LOC_HIP(hipSetDevice(w->device));
    // a resident launch (possibly on a caller's stream) may still be using the workspaces and tables this call shares with it
    if (int rc = wait_resident(w)) return rc;
    const size_t N = (size_t)n;
    const size_t out_bytes[2] = {N * locamd::table_bytes(c, kPoses), N * kResultBytes};   // what comes back: poses, result
    hipStream_t st = w->stream;
    // Single-block path: [poses | result | counts | r_val | p_val | s_val | r_idx | p_idx | s_idx], 16-byte aligned
    // pieces, sized for this call's n.  One H2D copy, one launch, one D2H copy of [poses | result]: a node's solve is
    // then ~0.2 ms of host/PCIe overhead around the kernel instead of a dozen small pageable copies.
    const locamd::BlockLayout L = locamd::pack_block(c, N, out_bytes, 2, kCounts);
    if (L.end <= kStageBytes) {
        if (int rc = ensure_stage(w)) return rc;
        char* h = w->h_stage; char* d = w->d_stage;
        locamd::stage_tables(h, L, c, b);
        const auto t_topo = clk::now();
        const int kind = host_kernel(w, b);
        w->t_topology_ms = ms_since(t_topo);
        const auto t_run = clk::now();
        // A handful of small windows on wave3_lm_kernel (the node's own solve): the kernel reads its few KB of input once and
        // writes 1 KB of results — it does so straight from / to the page-locked staging block (host-coherent memory, mapped
        // into the device's address space), which saves the two DMA operations around a ~75 us kernel.
        const size_t anchor_bytes = (size_t)w->n_anchors * 3 * sizeof(double);
        // (tree_wave_kernel likewise reads its inputs once, in its prologue — unless a pose has priors or more than two range edges, which it
        //  fetches from memory on every sweep: such windows are copied to the device first)
        const locamd::TreeSched& ts = w->slot[0].aux.tsched;
        const bool tree_once = kind == LOC_WINDOW_KERNEL_TREE && ts.np == 0 && ts.max_r_per_node <= 2 && ts.max_se3_per_node <= 1 && w->opt.tree != 2;
        const bool zero_copy = (kind == LOC_WINDOW_KERNEL_WAVE3 || kind == LOC_WINDOW_KERNEL_WAVE6 || kind == LOC_WINDOW_KERNEL_WAVE6S || tree_once) && n <= 4 && w->B <= 4 && w->h_anchors.size() == (size_t)w->n_anchors * 3 &&
                               L.end + anchor_bytes <= kStageBytes && w->opt.zero_copy;
        if (zero_copy) {
            d = h;
            if (anchor_bytes) std::memcpy(h + L.end, w->h_anchors.data(), anchor_bytes);
        } else {
            if (int rc = flush_anchors(w)) return rc;
            LOC_HIP(hipMemcpyAsync(d, h, L.end, hipMemcpyHostToDevice, st));
        }
        const locamd::WindowArgs a = window_args(w, locamd::tables_at(d, L), n, nullptr, zero_copy ? (const double*)(h + L.end) : w->d_anchors, (double*)(d + L.pre[1]));
        // (the two event records around a ~50 us kernel are not free; option "kernel_events" = 0 drops them for the zero-copy solve)
        const bool events = w->opt.kernel_events || !zero_copy;
        if (events) LOC_HIP(hipEventRecord(w->ev0, st));
        if (kind == LOC_WINDOW_KERNEL_ARROW3) LOC_HIP(upload_arrow_aux(w, w->slot[0], n, st));
        if (kind == LOC_WINDOW_KERNEL_TREE) LOC_HIP(upload_tree_sched(w, w->slot[0].aux, st));
        if (kind == LOC_WINDOW_KERNEL_TREE_GROUPS) LOC_HIP(upload_tree_sched(w, w->slot[0].aux, st, true, true));
        const auto t_launch = clk::now();
        hipError_t e = launch_any(w, w->slot[0], a, st, kind);
        if (e != hipSuccess) return locamd_fail_hip(e, "launch_window");
        if (events) LOC_HIP(hipEventRecord(w->ev1, st));
        if (!zero_copy) LOC_HIP(hipMemcpyAsync(h, d, L.tab[kCounts], hipMemcpyDeviceToHost, st));  // [poses | result]
        LOC_HIP(hipStreamSynchronize(st));
        float ms = (float)ms_since(t_launch);
        std::memcpy(poses, h + L.pre[0], out_bytes[0]);
        std::memcpy(result, h + L.pre[1], out_bytes[1]);
        if (events) LOC_HIP(hipEventElapsedTime(&ms, w->ev0, w->ev1));
        w->last_ms = ms;
        w->t_run_ms = ms_since(t_run);
        return LOC_OK;
    }
    if (int rc = flush_anchors(w)) return rc;
    // The large path stages its batch in the device arrays a resident batch lives in: that batch is gone from here on
    drop_resident(w);
    const auto t_topo = clk::now();
    const int kind = host_kernel(w, b);
    w->t_topology_ms = ms_since(t_topo);
    const auto t_run = clk::now();
    LOC_HIP(copy_tables(c, N, w->dev.t, b.tables().t, hipMemcpyHostToDevice, &st));
    const locamd::WindowArgs a = window_args(w, w->dev, n, nullptr, w->d_anchors, w->d_result);
    if (kind == LOC_WINDOW_KERNEL_ARROW3) LOC_HIP(upload_arrow_aux(w, w->slot[0], n, st));
    if (kind == LOC_WINDOW_KERNEL_TREE) LOC_HIP(upload_tree_sched(w, w->slot[0].aux, st));
    if (kind == LOC_WINDOW_KERNEL_TREE_GROUPS) LOC_HIP(upload_tree_sched(w, w->slot[0].aux, st, true, true));
    LOC_HIP(hipEventRecord(w->ev0, st));
    hipError_t e = launch_any(w, w->slot[0], a, st, kind);
    if (e != hipSuccess) return locamd_fail_hip(e, "launch_window");
    LOC_HIP(hipEventRecord(w->ev1, st));
    LOC_HIP(hipMemcpyAsync(poses, w->dev.t[kPoses], out_bytes[0], hipMemcpyDeviceToHost, st));
    LOC_HIP(hipMemcpyAsync(result, w->d_result, out_bytes[1], hipMemcpyDeviceToHost, st));
    LOC_HIP(hipStreamSynchronize(st));
    float ms = 0;
    LOC_HIP(hipEventElapsedTime(&ms, w->ev0, w->ev1));
    w->last_ms = ms;
    w->t_run_ms = ms_since(t_run);
    return LOC_OK;
}

// ---- device-resident operation --------------------------------------------------------------------------------------
int loc_window_upload(loc_window* w, int64_t n, const int32_t* counts, const double* poses, const int32_t* r_idx,
                      const double* r_val, const int32_t* p_idx, const double* p_val, const int32_t* s_idx,
                      const double* s_val) {
    const locamd::HostBatch b{n, poses, counts, r_val, p_val, s_val, r_idx, p_idx, s_idx};
    if (int rc = validate_instances(w, b)) return rc;
    const locamd::WindowCaps& c = w->caps;
    LOC_HIP(hipSetDevice(w->device));
    // a resident launch of the previous batch may still be running on the handle's (or the caller's) stream: it reads what the
    // copies below overwrite
    LOC_HIP(hipStreamSynchronize(w->stream));
    if (int rc = wait_resident(w)) return rc;
    // (a failing step below must not leave a half-described resident batch behind: nothing is resident until everything is)
    drop_resident(w);   // (and its covariance verdict with it)
    Resident& R = w->res;
    if (!w->d_poses_in) LOC_HIP(hipMalloc((void**)&w->d_poses_in, (size_t)w->B * locamd::table_bytes(c, kPoses)));
    LOC_HIP(copy_tables(c, (size_t)n, uploaded_tables(w).t, b.tables().t, hipMemcpyHostToDevice, nullptr));
    loc_window::BatchSlot& S = w->slot[1];
    const int topology = locamd::batch_topology(c, w->opt, w->fits, w->n_anchors, b, S.aux, nullptr).kind;
    if (topology == LOC_WINDOW_KERNEL_ARROW3) LOC_HIP(upload_arrow_aux(w, S, n, w->stream));
    if (topology == LOC_WINDOW_KERNEL_TREE) LOC_HIP(upload_tree_sched(w, S.aux, w->stream));
    // (the grouped forest: its covariance verdict stays open — the first covariance call takes it under the options as they are then; what
    //  that call needs to walk the block just uploaded without a copy-back is noted here: the batch is no chain in any edge order)
    if (topology == LOC_WINDOW_KERNEL_TREE_GROUPS) {
        LOC_HIP(upload_tree_sched(w, S.aux, w->stream, true, true));
        bool chain = false, single_pairs = false, se3_pairs = false;
        locamd::chain_scan(c, b, false, chain, single_pairs, se3_pairs);
        R.groups_no_chain = !chain;
    }
    note_groups(w, S.aux, topology);
    R.min_anchors = locamd::max_anchor_referenced(c, n, counts, r_idx);
    R.counts.assign(counts, counts + (size_t)n * 4);
    if (w->opt_slide) {   // the mirror of loc_window_slide_resident
        R.mir_ridx.assign((size_t)n * c.nr_max * 2, 0);
        R.mir_pidx.assign((size_t)n * c.np_max, 0);
        if (c.nr_max) std::memcpy(R.mir_ridx.data(), r_idx, R.mir_ridx.size() * sizeof(int32_t));
        if (c.np_max) std::memcpy(R.mir_pidx.data(), p_idx, R.mir_pidx.size() * sizeof(int32_t));
        R.mirror_valid = true;
    }
    R.topology = topology;
    R.skip = locamd::structured_pinfo(w->opt);
    // the pass of loc_window_covariance_resident: ordered chain batches are known from the verdict above; any other batch is
    // classified by the first loc_window_covariance_resident call (an upload costs nothing more for callers that never ask)
    if (topology == LOC_WINDOW_KERNEL_CHAIN3) R.cov = CovKind::Chain3;
    else if (topology == LOC_WINDOW_KERNEL_CHAIN || topology == LOC_WINDOW_KERNEL_WAVE6 || topology == LOC_WINDOW_KERNEL_WAVE6S) R.cov = CovKind::Chain6;
    else if (topology == LOC_WINDOW_KERNEL_TREE) {
        // a forest the solve kernels take: the covariance pass walks the schedule just built and uploaded (S.aux) — unless the batch is
        // a chain in some edge order, which the chain pass serves as before
        bool chain = false, single_pairs = false, se3_pairs = false;
        locamd::chain_scan(c, b, false, chain, single_pairs, se3_pairs);
        R.cov = chain ? CovKind::Unclassified : CovKind::Forest;
    } else if (topology == LOC_WINDOW_KERNEL_ARROW3) {   // (never a chain: build_arrow_aux wants a border)
        R.cov = CovKind::Arrow;
        S.cov_list_cap = S.aux.arrow_list_cap;
    } else R.cov = CovKind::Unclassified;
    R.n = n;
    return LOC_OK;
}

// Option "upload_dev_structures": batch_topology's two tests behind its chain block — the arrowhead, then the forest, each under its
// conditions — for an admitted batch that is no chain and already lies in the handle's device arrays (window_structure_kernel.hip; DESIGN.md
// §2, "Upload from device arrays").  One launch pair answers both tests and the host reads back ONE record; an arrowhead batch is packed by a
// further launch at the sizes of that record, a forest batch sends window 0's counts and index rows (one window, not the batch) to
// build_tree_sched.  topology / cov: what loc_window_upload of the same arrays leaves in Resident — untouched when neither test takes the
// batch.  slot[1].aux is written here alone, after the previous batch was dropped.  The launches end the call's cov_ev0 / cov_ev1 bracket:
// cov_ev1 is recorded again behind them, so loc_window_last_covariance_ms spans admission, copy and these launches.
// mixed: the forest test ran, neither test took the batch, and the windows are NOT all equal to window 0 (what dev_forest_groups below is for).
static int dev_structures(loc_window* w, int64_t n, const locamd::WindowBatchFlags& flags, hipStream_t st, int& topology, CovKind& cov, bool& mixed) {
    mixed = false;
    const locamd::WindowCaps& c = w->caps;
    const locamd::DispatchOpts& o = w->opt;
    loc_window::BatchSlot& S = w->slot[1];
    locamd::WinAux& A = S.aux;
    // (arrow3_fits grows with the border: a handle that fails it for a border of one row fails it for every batch)
    const bool arrow = locamd::arrow3_wanted(o, w->fits) && flags.translation_only && locamd::arrow3_fits(c, 1);
    const bool forest = o.tree != 0 && n >= locamd::tree_min_batch(o) && !locamd::general_only(o);   // (build_tree_sched refuses under general_only)
    if (!arrow && !forest) return LOC_OK;
    const size_t at_record = (size_t)locamd::kStructMaxWaves * sizeof(locamd::WindowStructRecord);
    if (!w->d_struct) LOC_HIP(hipMalloc((void**)&w->d_struct, at_record + sizeof(locamd::WindowStructRecord)));
    if (!w->h_struct_record) LOC_HIP(hipHostMalloc((void**)&w->h_struct_record, sizeof(locamd::WindowStructRecord), hipHostMallocDefault));
    if (arrow) LOC_HIP(reserve_arrow_rows(w, A));
    const locamd::DeviceTables& d = w->dev;
    locamd::WindowStructArgs a{};
    a.counts = (const int32_t*)d.t[kCounts]; a.r_idx = (const int32_t*)d.t[locamd::kRIdx]; a.p_idx = (const int32_t*)d.t[locamd::kPIdx]; a.s_idx = (const int32_t*)d.t[locamd::kSIdx];
    a.hdr = A.d_ahdr; a.rslot = A.d_arslot;
    a.partial = (locamd::WindowStructRecord*)w->d_struct; a.record = (locamd::WindowStructRecord*)(w->d_struct + at_record);
    a.arrow = arrow; a.forest = forest; a.B = n; a.caps = c;
    LOC_HIP(locamd::launch_window_structure(a, st));
    LOC_HIP(hipEventRecord(w->cov_ev1, st));
    LOC_HIP(hipMemcpyAsync(w->h_struct_record, a.record, sizeof(locamd::WindowStructRecord), hipMemcpyDeviceToHost, st));
    LOC_HIP(hipStreamSynchronize(st));
    const locamd::WindowStructRecord rec = *w->h_struct_record;
    const locamd::ArrowMaxima& m = rec.arrow;
    if (arrow && (rec.and_bits & locamd::kStructArrow) != 0 && !locamd::arrow_batch_refused(m) && locamd::arrow3_fits(c, m.nb_max)) {
        const int nchunk = (c.nv_max + 63) / 64;
        A.arrow_nb_max = m.nb_max; A.arrow_jmax = m.jmax; A.arrow_jpmax = m.jpmax; A.arrow_list_cap = m.list_cap;
        for (int k = 0; k < 16; ++k) { A.arrow_jch[k] = m.jch[k]; A.arrow_jpch[k] = m.jpch[k]; }
        LOC_HIP(reserve_arrow_records(w, A, n, (size_t)n * locamd::arrow_rec_doubles(nchunk, m.jmax), (size_t)n * locamd::arrow_prec_doubles(nchunk, m.jpmax)));
        locamd::ArrowPackArgs p{};
        p.counts = a.counts; p.r_idx = a.r_idx; p.r_val = (const double*)d.t[locamd::kRVal]; p.p_idx = a.p_idx; p.p_val = (const double*)d.t[locamd::kPVal];
        p.hdr = A.d_ahdr; p.rec = A.d_arec; p.prec = A.d_aprec; p.jmax = m.jmax; p.jpmax = m.jpmax; p.nchunk = nchunk; p.B = n; p.caps = c;
        LOC_HIP(locamd::launch_window_arrow_pack(p, st));
        LOC_HIP(hipEventRecord(w->cov_ev1, st));
        LOC_HIP(hipStreamSynchronize(st));
        topology = LOC_WINDOW_KERNEL_ARROW3;
        cov = CovKind::Arrow;
        S.cov_list_cap = m.list_cap;
        return LOC_OK;
    }
    if (forest && (rec.and_bits & locamd::kStructEqual0) != 0) {
        // every window equals window 0: everything else build_tree_sched reads is window 0's integer tables
        int32_t cn[4];
        LOC_HIP(hipMemcpy(cn, d.t[kCounts], sizeof(cn), hipMemcpyDeviceToHost));
        std::vector<int32_t> ridx((size_t)cn[1] * 2), pidx((size_t)cn[2]), sidx((size_t)cn[3] * 4);
        if (!ridx.empty()) LOC_HIP(hipMemcpy(ridx.data(), d.t[locamd::kRIdx], ridx.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (!pidx.empty()) LOC_HIP(hipMemcpy(pidx.data(), d.t[locamd::kPIdx], pidx.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (!sidx.empty()) LOC_HIP(hipMemcpy(sidx.data(), d.t[locamd::kSIdx], sidx.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        const locamd::HostBatch one{1, nullptr, cn, nullptr, nullptr, nullptr, ridx.data(), pidx.data(), sidx.data()};
        if (locamd::build_tree_sched(c, locamd::general_only(o), one, A)) {
            LOC_HIP(upload_tree_sched(w, A, w->stream));
            bool chain = false, single_pairs = false, se3_pairs = false;
            locamd::chain_scan(c, one, false, chain, single_pairs, se3_pairs);   // (the batch's: every window has window 0's rows)
            topology = LOC_WINDOW_KERNEL_TREE;
            cov = chain ? CovKind::Unclassified : CovKind::Forest;
        }
    }
    mixed = forest && (rec.and_bits & locamd::kStructEqual0) == 0;
    return LOC_OK;
}

// Option "upload_dev_forest_groups": batch_topology's last test, build_tree_groups, for an admitted batch that dev_structures found to be
// neither an arrowhead nor of one topology and that forest_groups_wanted admits (window_groups_kernel.hip; DESIGN.md §2, "Upload from device
// arrays").  The windows are grouped by topology key on the device; the host reads ONE record, then sched_of (4 bytes per window) and the G
// representatives' counts and used index rows, and part (b) of build_tree_groups (build_tree_groups_block) builds the block that
// loc_window_upload of the same arrays builds — byte for byte, refusals included.  A hash collision or a table overflow (the record says so)
// fetches the batch's counts and index tables and calls build_tree_groups itself: rare, and always exact.  topology / groups_no_chain: what
// loc_window_upload leaves in Resident; slot[1].aux describes no groups when the batch is refused.  The launches sit inside the call's
// cov_ev0 / cov_ev1 bracket: cov_ev1 is recorded again behind the last of them.
static int dev_forest_groups(loc_window* w, int64_t n, hipStream_t st, int& topology, bool& groups_no_chain) {
    const locamd::WindowCaps& c = w->caps;
    const locamd::DispatchOpts& o = w->opt;
    locamd::WinAux& A = w->slot[1].aux;
    A.n_groups = 0;
    A.h_groups.clear();
    const size_t B = (size_t)w->B, N = (size_t)n;
    // the pass's block: hash u64 [B] | tab_key u64 [slots] | tab_inv u32 [slots] | rep0, sched_of, rep i32 [B] each | kGroupsMaxWaves partial records | the record
    const uint64_t slots = locamd::groups_table_slots(w->B);
    const size_t at_key = B * sizeof(uint64_t), at_inv = at_key + slots * sizeof(uint64_t), at_rep0 = at_inv + slots * sizeof(uint32_t), at_of = at_rep0 + B * sizeof(int32_t),
                 at_rep = at_of + B * sizeof(int32_t), at_partial = (at_rep + B * sizeof(int32_t) + 7) / 8 * 8,
                 at_record = at_partial + (size_t)locamd::kGroupsMaxWaves * sizeof(locamd::WindowGroupsRecord);
    if (!w->d_groups_pass) LOC_HIP(hipMalloc((void**)&w->d_groups_pass, at_record + sizeof(locamd::WindowGroupsRecord)));
    if (!w->h_groups_record) LOC_HIP(hipHostMalloc((void**)&w->h_groups_record, sizeof(locamd::WindowGroupsRecord), hipHostMallocDefault));
    const locamd::DeviceTables& d = w->dev;
    char* blk = w->d_groups_pass;
    locamd::WindowGroupsArgs a{};
    a.counts = (const int32_t*)d.t[kCounts]; a.r_idx = (const int32_t*)d.t[locamd::kRIdx]; a.p_idx = (const int32_t*)d.t[locamd::kPIdx]; a.s_idx = (const int32_t*)d.t[locamd::kSIdx];
    a.hash = (uint64_t*)blk; a.tab_key = (uint64_t*)(blk + at_key); a.tab_inv = (uint32_t*)(blk + at_inv); a.slots = slots;
    a.rep0 = (int32_t*)(blk + at_rep0); a.sched_of = (int32_t*)(blk + at_of); a.rep = (int32_t*)(blk + at_rep);
    a.partial = (locamd::WindowGroupsRecord*)(blk + at_partial); a.record = (locamd::WindowGroupsRecord*)(blk + at_record);
    a.hash_bits = o.upload_dev_groups_hash_bits; a.B = n; a.caps = c;
    LOC_HIP(locamd::launch_window_groups(a, st));
    LOC_HIP(hipEventRecord(w->cov_ev1, st));
    LOC_HIP(hipMemcpyAsync(w->h_groups_record, a.record, sizeof(locamd::WindowGroupsRecord), hipMemcpyDeviceToHost, st));
    LOC_HIP(hipStreamSynchronize(st));
    const locamd::WindowGroupsRecord rec = *w->h_groups_record;
    if ((rec.or_bits & locamd::kGroupsBadNv) != 0) return LOC_OK;   // (build_tree_groups refuses a window with nv outside [2, 64]: the general kernel)
    bool ok = false, chain = false, single_pairs = false, se3_pairs = false;
    if ((rec.or_bits & (locamd::kGroupsCollision | locamd::kGroupsOverflow)) != 0 || rec.n_groups < 1 || rec.n_groups > n) {
        std::vector<int32_t> counts(N * 4), ridx(N * c.nr_max * 2), pidx(N * c.np_max), sidx(N * c.ns_max * 4);
        LOC_HIP(hipMemcpy(counts.data(), a.counts, counts.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (!ridx.empty()) LOC_HIP(hipMemcpy(ridx.data(), a.r_idx, ridx.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (!pidx.empty()) LOC_HIP(hipMemcpy(pidx.data(), a.p_idx, pidx.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (!sidx.empty()) LOC_HIP(hipMemcpy(sidx.data(), a.s_idx, sidx.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        const locamd::HostBatch all{n, nullptr, counts.data(), nullptr, nullptr, nullptr, ridx.data(), pidx.data(), sidx.data()};
        ok = locamd::build_tree_groups(c, locamd::general_only(o), all, A);
        if (ok) locamd::chain_scan(c, all, false, chain, single_pairs, se3_pairs);
    } else {
        const size_t G = (size_t)rec.n_groups;
        const size_t per = 4 + (size_t)c.nr_max * 2 + c.np_max + (size_t)c.ns_max * 4;   // int32s of one window's compact rows
        LOC_HIP(locamd::grow_buffers(w->groups_compact_cap, G, {{w->d_groups_compact, G * per * sizeof(int32_t)}}));
        const size_t cap = w->groups_compact_cap;   // (the tables are laid out for the buffer's capacity, not for G)
        locamd::WindowGroupsGatherArgs g{};
        g.counts = a.counts; g.r_idx = a.r_idx; g.p_idx = a.p_idx; g.s_idx = a.s_idx; g.rep = a.rep;
        g.c_counts = w->d_groups_compact; g.c_r_idx = g.c_counts + cap * 4; g.c_p_idx = g.c_r_idx + cap * c.nr_max * 2; g.c_s_idx = g.c_p_idx + cap * c.np_max;
        g.G = (long long)G; g.B = n; g.caps = c;
        LOC_HIP(locamd::launch_window_groups_gather(g, st));
        LOC_HIP(hipEventRecord(w->cov_ev1, st));
        std::vector<int32_t> of(N), counts(G * 4), ridx(G * c.nr_max * 2), pidx(G * c.np_max), sidx(G * c.ns_max * 4);
        LOC_HIP(hipMemcpyAsync(of.data(), a.sched_of, of.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        LOC_HIP(hipMemcpyAsync(counts.data(), g.c_counts, counts.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        if (!ridx.empty()) LOC_HIP(hipMemcpyAsync(ridx.data(), g.c_r_idx, ridx.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        if (!pidx.empty()) LOC_HIP(hipMemcpyAsync(pidx.data(), g.c_p_idx, pidx.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        if (!sidx.empty()) LOC_HIP(hipMemcpyAsync(sidx.data(), g.c_s_idx, sidx.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        LOC_HIP(hipStreamSynchronize(st));
        const locamd::HostBatch reps{(int64_t)G, nullptr, counts.data(), nullptr, nullptr, nullptr, ridx.data(), pidx.data(), sidx.data()};
        ok = locamd::build_tree_groups_block(c, locamd::general_only(o), reps, n, of.data(), A);
        // (chain_scan(ordered = false) reads a window's counts, the sign of v1 and |v0 - v1| of its range rows and columns 0 - 1 of its EdgeSE3
        //  rows: all of them words of the topology key, and the batch's verdict is the AND over its windows — the representatives answer for the batch)
        if (ok) locamd::chain_scan(c, reps, false, chain, single_pairs, se3_pairs);
    }
    if (!ok) return LOC_OK;
    LOC_HIP(upload_tree_sched(w, A, w->stream, true, true));
    topology = LOC_WINDOW_KERNEL_TREE_GROUPS;
    groups_no_chain = !chain;
    return LOC_OK;
}

// The same from the caller's DEVICE arrays ("Upload from device arrays"): window_admit_kernel.hip admits every window and scans
// the chain family's structure on hip_stream, the host reads back one record (the call's ONE synchronisation of that stream), and an admitted
// batch is copied device-to-device.  A refused batch copies nothing and leaves the previous resident batch as it was.  The host copies of the
// integer tables are not made: they are sized and marked stale (refresh_mirror).  Option "upload_dev_structures": a batch that is no chain
// goes on to dev_structures above, and what that leaves of mixed forest windows, under option "upload_dev_forest_groups", to dev_forest_groups.
int loc_window_upload_dev(loc_window* w, void* hip_stream, int64_t n, const void* counts_dev, const void* poses_dev, const void* r_idx_dev, const void* r_val_dev,
                          const void* p_idx_dev, const void* p_val_dev, const void* s_idx_dev, const void* s_val_dev, void* admit_dev) {
    const locamd::HostBatch b{n, (const double*)poses_dev, (const int32_t*)counts_dev, (const double*)r_val_dev, (const double*)p_val_dev, (const double*)s_val_dev,
                              (const int32_t*)r_idx_dev, (const int32_t*)p_idx_dev, (const int32_t*)s_idx_dev};
    if (int rc = validate_arguments(w, b)) return rc;
    const locamd::WindowCaps& c = w->caps;
    hipStream_t st;
    if (int rc = resident_stream(w, hip_stream, false, st)) return rc;
    const size_t B = (size_t)w->B;
    // the admit block: flags [B] | kAdmitMaxWaves partial records | the record (every part a multiple of 8 bytes)
    const size_t at_partial = B * sizeof(uint64_t), at_record = at_partial + (size_t)locamd::kAdmitMaxWaves * sizeof(locamd::WindowAdmitRecord);
    if (!w->d_admit) LOC_HIP(hipMalloc((void**)&w->d_admit, at_record + sizeof(locamd::WindowAdmitRecord)));
    if (!w->h_admit_record) LOC_HIP(hipHostMalloc((void**)&w->h_admit_record, sizeof(locamd::WindowAdmitRecord), hipHostMallocDefault));
    locamd::WindowAdmitArgs a{};
    a.counts = b.counts; a.poses = b.poses; a.r_idx = b.r_idx; a.r_val = b.r_val; a.p_idx = b.p_idx; a.p_val = b.p_val; a.s_idx = b.s_idx;
    a.admit = (int32_t*)admit_dev; a.flags = (uint64_t*)w->d_admit;
    a.partial = (locamd::WindowAdmitRecord*)(w->d_admit + at_partial); a.record = (locamd::WindowAdmitRecord*)(w->d_admit + at_record);
    a.n_anchors = w->n_anchors; a.B = n; a.caps = c;
    // (the pass reads the caller's arrays and writes the handle's admit block alone: no resident array, so it does not wait for resident work)
    // (between cov_ev0 and cov_ev1, as the slides' launches are: loc_window_last_covariance_ms reports the pass's two launches)
    LOC_HIP(hipEventRecord(w->cov_ev0, st));
    LOC_HIP(locamd::launch_window_admit(a, st));
    LOC_HIP(hipEventRecord(w->cov_ev1, st));
    w->cov_pending = true;
    LOC_HIP(hipMemcpyAsync(w->h_admit_record, a.record, sizeof(locamd::WindowAdmitRecord), hipMemcpyDeviceToHost, st));
    LOC_HIP(hipStreamSynchronize(st));
    const locamd::WindowAdmitRecord rec = *w->h_admit_record;
    if (rec.first_bad != locamd::kWinNoneRefused) {
        const int code = rec.code >= 1 && rec.code <= 6 ? rec.code : 1;
        char text[160];
        std::snprintf(text, sizeof(text), "%s (window %lld)", kInstanceCheck[code], rec.first_bad);
        return locamd_fail(LOC_ERR_INVALID, text);
    }
    // as loc_window_upload from here: a resident launch of the previous batch may still read what the copies below overwrite
    LOC_HIP(hipStreamSynchronize(w->stream));
    if (int rc = wait_resident(w)) return rc;
    drop_resident(w);
    Resident& R = w->res;
    if (!w->d_poses_in) LOC_HIP(hipMalloc((void**)&w->d_poses_in, B * locamd::table_bytes(c, kPoses)));
    LOC_HIP(copy_tables(c, (size_t)n, uploaded_tables(w).t, b.tables().t, hipMemcpyDeviceToDevice, &st));
    LOC_HIP(hipStreamSynchronize(st));   // (the call returns synchronously, like loc_window_upload: the caller's arrays are free again)
    const locamd::WindowBatchFlags flags = locamd::window_batch_flags(rec);
    int topology = locamd::topology_from_flags(w->opt, w->fits, flags);
    CovKind cov = topology == LOC_WINDOW_KERNEL_CHAIN3 ? CovKind::Chain3 : topology == LOC_WINDOW_KERNEL_GENERAL ? CovKind::Unclassified : CovKind::Chain6;
    bool groups_no_chain = false;
    if (w->opt.upload_dev_structures && !flags.chain) {
        bool mixed = false;
        if (int rc = dev_structures(w, n, flags, st, topology, cov, mixed)) return rc;
        if (mixed && topology == LOC_WINDOW_KERNEL_GENERAL && w->opt.upload_dev_forest_groups && locamd::forest_groups_wanted(w->opt, c, n))
            if (int rc = dev_forest_groups(w, n, st, topology, groups_no_chain)) return rc;
    }
    R.groups_no_chain = groups_no_chain;
    R.min_anchors = rec.max_anchor;
    R.counts.assign((size_t)n * 4, 0);
    if (w->opt_slide) {
        R.mir_ridx.assign((size_t)n * c.nr_max * 2, 0);
        R.mir_pidx.assign((size_t)n * c.np_max, 0);
        R.mirror_valid = true;
    }
    R.mirror_stale = true;   // (refresh_mirror: the first reader of counts or the mirror fetches them)
    note_groups(w, w->slot[1].aux, topology);   // (the grouped path under option "upload_dev_forest_groups" alone)
    R.topology = topology;
    R.skip = locamd::structured_pinfo(w->opt);
    R.cov = cov;
    R.n = n;
    return LOC_OK;
}

int loc_window_solve_resident(loc_window* w, void* hip_stream) {
    if (int rc = resident_gate(w, locamd::ResidentEntry::Solve)) return rc;
    const int rc = resident_launch(w, hip_stream, Timing::Solve, true, [&](hipStream_t st) {
        const locamd::WindowArgs a = window_args(w, w->dev, w->res.n, w->d_poses_in, w->d_anchors, w->d_result);
        // (the batch-size threshold and the ordering override are looked at per solve: loc_window_set_chain_threshold /
        //  loc_window_set_ordering after the upload take effect)
        return launched(launch_any(w, w->slot[1], a, st, locamd::pick_kernel(w->opt, w->fits, w->res.n, resident_topology(w))), "launch_window");
    });
    if (rc == LOC_OK) w->res.solved = true;
    return rc;
}

int loc_window_download(loc_window* w, double* poses, double* result) {
    if (int rc = resident_gate(w, locamd::ResidentEntry::Download)) return rc;
    LOC_HIP(hipSetDevice(w->device));
    if (int rc = wait_resident(w)) return rc;
    const size_t N = (size_t)w->res.n;
    if (poses) LOC_HIP(hipMemcpy(poses, w->dev.t[kPoses], N * locamd::table_bytes(w->caps, kPoses), hipMemcpyDeviceToHost));
    if (result) LOC_HIP(hipMemcpy(result, w->d_result, N * kResultBytes, hipMemcpyDeviceToHost));
    return LOC_OK;
}

void* loc_window_poses_device(loc_window* w) { return w ? w->dev.t[kPoses] : nullptr; }
void* loc_window_result_device(loc_window* w) { return w ? (void*)w->d_result : nullptr; }

int loc_window_timing_begin(loc_window* w, int32_t max_launches) {
    return w ? w->timer.begin(w->device, max_launches) : locamd_fail(LOC_ERR_INVALID, "timing_begin");
}
int loc_window_timing_end(loc_window* w, int32_t* n_launches, double* total_ms, double* avg_ms) {
    return w ? w->timer.end(w->device, n_launches, total_ms, avg_ms) : locamd_fail(LOC_ERR_INVALID, "timing_end");
}

int loc_window_last_covariance_kind(const loc_window* w, int32_t* kind) {
    if (!w || !kind) return locamd_fail(LOC_ERR_INVALID, "null");
    *kind = w->last_cov_kind;
    return LOC_OK;
}

int loc_window_last_kernel_ms(loc_window* w, double* ms) {
    if (!w || !ms) return locamd_fail(LOC_ERR_INVALID, "null");
    *ms = w->last_ms;
    return LOC_OK;
}

// ---- marginal covariances (covariance_kernel.hip: chains; arrow_covariance_kernel.hip: arrowheads; forest_covariance_kernel.hip: forests) -------------------------------------------------------------------------------------
#define LOC_COV_UNSUPPORTED ": every window must be a chain of <= 64 poses, or the batch an arrowhead that the handle solves on arrow3_lm_kernel (option arrow3), " \
                            "or a forest of one shared topology of <= 64 poses that the handle solves on a forest kernel (option tree, batch threshold), " \
                            "or forests of differing topologies that the handle solves on the grouped forest kernel with options forest_groups and forest_groups_covariance both 1, " \
                            "or option covariance_general must be 1 (any structure and length, in the caller's pose order: the only pass for full-information priors); no endpoint-1 lever arms"

// the pass of a batch of covariance_kind's `kind`; S: the batch's table sets and workspaces (a forest that loc_window_upload classified,
// Forest, walks the resident solve's schedule slot[1].aux; ForestOwn the covariance's own, S.cov_aux; ForestGroups / ForestGroupsOwn likewise
// the groups block of the resident solve / of the covariance's own)
// env_blocks: the envelope the workspace was sized for (a joint call's includes its pairs); pp: the pairs on the device, cross = nullptr for none
static hipError_t launch_covariance(loc_window* w, loc_window::BatchSlot& S, CovKind kind, long long env_blocks, const locamd::WindowArgs& a, double* cov, int32_t* mask,
                                    int32_t* status, const locamd::CovPairs& pp, hipStream_t st) {
    if (kind == CovKind::Arrow) return locamd::launch_window_arrow_covariance(a, S.d_cov_ws, S.cov_list_cap, cov, mask, status, pp, st);
    if (kind == CovKind::Envelope) return locamd::launch_window_envelope_covariance(a, S.d_env_ws, env_blocks, cov, mask, status, pp, st);
    if (kind == CovKind::Forest) return locamd::launch_window_forest_covariance(a, w->slot[1].aux.tsched, cov, mask, status, pp, st);
    if (kind == CovKind::ForestOwn) return locamd::launch_window_forest_covariance(a, S.cov_aux.tsched, cov, mask, status, pp, st);
    if (kind == CovKind::ForestGroups || kind == CovKind::ForestGroupsOwn) {
        const locamd::WinAux& A = kind == CovKind::ForestGroups ? w->slot[1].aux : S.cov_aux;
        if (A.n_groups <= 0 || !A.d_groups) return hipErrorInvalidValue;
        const locamd::TreeGroups g{A.d_groups, A.d_groups + A.groups_of_at, A.d_groups + A.groups_tab_at, A.n_groups};
        return locamd::launch_window_forest_covariance_groups(a, g, A.h_groups.data(), cov, mask, status, pp, st);
    }
    return locamd::launch_window_covariance(a, kind == CovKind::Chain3, cov, mask, status, pp, st);
}
// the pair arguments of a joint call as given (npair_max = 0: none, the plain call): 0, or the error
static int validate_pairs(int64_t n, const int32_t* counts, const locamd::PairTables& pt, const void* cross) {
    if (pt.npair_max < 0 || (pt.npair_max > 0 && (!pt.counts || !pt.pairs || !cross))) return locamd_fail(LOC_ERR_INVALID, "joint covariance: pair arrays");
    static const char* const kWhat[] = {nullptr, "joint covariance: a pair count outside [0, npair_max]", "joint covariance: a pair names a pose slot outside its window"};
    if (const int bad = locamd::check_pairs(n, counts, pt)) return locamd_fail(LOC_ERR_INVALID, kWhat[bad]);
    return LOC_OK;
}
// The synchronous host calls beside the solve (joint covariance, marginal prior) as ONE pipeline.  L: the call's block — its output pieces,
// then its extra input pieces, then all eight tables of b.  ins / outs: the caller's arrays and the prefix piece each travels in (a null
// array: the call has no such piece).  Small calls go through the staging block of loc_window_solve_host (free between calls, never used by a
// resident launch), large ones through a device block of the covariance's own: the resident batch's arrays are not touched.
// launch(a, d, st): the kernel on the tables at device base d; cov_ev0 / cov_ev1 around it give loc_window_last_covariance_ms.
extern "C++" {   // (a template cannot have C linkage)
struct PieceIn { const void* p; int k; };
struct PieceOut { void* p; int k; };
template <class Launch>
static int staged_call(loc_window* w, const locamd::BlockLayout& L, const locamd::HostBatch& b, std::initializer_list<PieceIn> ins, std::initializer_list<PieceOut> outs,
                       const char* what, Launch&& launch) {
    size_t in0 = L.tab[kPoses];   // the outputs end and the inputs begin here
    for (const PieceIn& i : ins) if (i.p) in0 = std::min(in0, L.pre[i.k]);
    hipStream_t st = w->stream;
    char* d;
    const bool small = L.end <= kStageBytes;
    if (small) {
        if (int rc = ensure_stage(w)) return rc;
        locamd::stage_tables(w->h_stage, L, w->caps, b);
        for (const PieceIn& i : ins) if (i.p) std::memcpy(w->h_stage + L.pre[i.k], i.p, L.len[i.k]);
        d = w->d_stage;
        LOC_HIP(hipMemcpyAsync(d + in0, w->h_stage + in0, L.end - in0, hipMemcpyHostToDevice, st));
    } else {
        LOC_HIP(locamd::grow_buffers(w->cov_cap, L.end, {{w->d_cov, L.end}}));
        d = w->d_cov;
        LOC_HIP(copy_tables(w->caps, (size_t)b.n, locamd::tables_at(d, L).t, b.tables().t, hipMemcpyHostToDevice, &st));
        for (const PieceIn& i : ins) if (i.p) LOC_HIP(hipMemcpyAsync(d + L.pre[i.k], i.p, L.len[i.k], hipMemcpyHostToDevice, st));
    }
    const locamd::WindowArgs a = window_args(w, locamd::tables_at(d, L), b.n, nullptr, w->d_anchors, nullptr);
    LOC_HIP(hipEventRecord(w->cov_ev0, st));
    const hipError_t e = launch(a, d, st);
    if (e != hipSuccess) return locamd_fail_hip(e, what);
    LOC_HIP(hipEventRecord(w->cov_ev1, st));
    if (small) {
        LOC_HIP(hipMemcpyAsync(w->h_stage, d, in0, hipMemcpyDeviceToHost, st));   // every output piece in one copy
        LOC_HIP(hipStreamSynchronize(st));
        for (const PieceOut& o : outs) if (o.p) std::memcpy(o.p, w->h_stage + L.pre[o.k], L.len[o.k]);
    } else {
        for (const PieceOut& o : outs) if (o.p) LOC_HIP(hipMemcpyAsync(o.p, d + L.pre[o.k], L.len[o.k], hipMemcpyDeviceToHost, st));
        LOC_HIP(hipStreamSynchronize(st));
    }
    float ms = 0;
    LOC_HIP(hipEventElapsedTime(&ms, w->cov_ev0, w->cov_ev1));
    w->cov_ms = ms;
    w->cov_pending = false;
    return LOC_OK;
}
}  // extern "C++"
// loc_window_covariance_host is the joint call without pairs (pt.npair_max = 0, cross = nullptr): one staging, classification and launch path
int loc_window_joint_covariance_host(loc_window* w, int64_t n, const int32_t* counts, const double* poses, const int32_t* r_idx, const double* r_val,
                                     const int32_t* p_idx, const double* p_val, const int32_t* s_idx, const double* s_val,
                                     int32_t npair_max, const int32_t* pair_counts, const int32_t* pairs,
                                     double* cov, int32_t* mask, int32_t* status, double* cross) {
    if (!cov || !mask || !status) return locamd_fail(LOC_ERR_INVALID, "covariance output arrays");
    const locamd::HostBatch b{n, poses, counts, r_val, p_val, s_val, r_idx, p_idx, s_idx};
    if (int rc = validate_instances(w, b)) return rc;
    const locamd::PairTables pt{npair_max, pair_counts, pairs};
    if (int rc = validate_pairs(n, counts, pt, cross)) return rc;
    const bool joint = npair_max > 0;
    const locamd::WindowCaps& c = w->caps;
    loc_window::BatchSlot& S = w->slot[0];
    const locamd::CovVerdict v = locamd::covariance_kind(c, w->opt, w->fits, w->n_anchors, b, pt, S.cov_aux, &w->cov_sched);
    const CovKind kind = v.kind;
    if (kind == CovKind::None) return locamd_fail(LOC_ERR_UNSUPPORTED, "loc_window_covariance_host" LOC_COV_UNSUPPORTED);
    S.cov_list_cap = v.list_cap; S.env_blocks = v.env_blocks;
    LOC_HIP(hipSetDevice(w->device));
    if (kind == CovKind::Arrow) LOC_HIP(grow_cov_workspace(w, S, n, S.cov_list_cap));
    if (kind == CovKind::Envelope) LOC_HIP(grow_env_workspace(w, S, n, S.env_blocks));
    if (v.need_upload) {
        LOC_HIP(upload_tree_sched(w, S.cov_aux, w->stream, false, kind == CovKind::ForestGroupsOwn));
        w->cov_sched.valid = true;
    }
    if (int rc = flush_anchors(w)) return rc;
    const locamd::BlockLayout L = locamd::covariance_layout(c, (size_t)n, (size_t)npair_max);
    // (a plain call's block has no piece 3 .. 5, whatever the caller passed for them)
    const int rc = staged_call(w, L, b, {{joint ? pair_counts : nullptr, 4}, {joint ? pairs : nullptr, 5}}, {{cov, 0}, {mask, 1}, {status, 2}, {joint ? cross : nullptr, 3}}, "launch_window_covariance",
                       [&](const locamd::WindowArgs& a, char* d, hipStream_t st) {
        const locamd::CovPairs pp = joint ? locamd::CovPairs{(const int32_t*)(d + L.pre[4]), (const int32_t*)(d + L.pre[5]), (double*)(d + L.pre[3]), npair_max}
                                          : locamd::CovPairs{nullptr, nullptr, nullptr, 0};
        return launch_covariance(w, S, kind, S.env_blocks, a, (double*)(d + L.pre[0]), (int32_t*)(d + L.pre[1]), (int32_t*)(d + L.pre[2]), pp, st);
    });
    if (rc == LOC_OK) w->last_cov_kind = locamd::cov_public_kind(kind);
    return rc;
}

// ---- the marginal prior of a dropped pose (marginal_prior_kernel.hip) ------------------------------------------------------------
// stateless and synchronous (staged_call: the resident batch's arrays are not touched)
int loc_window_marginal_prior_host(loc_window* w, int64_t n, const int32_t* counts, const double* poses, const int32_t* r_idx, const double* r_val,
                                   const int32_t* p_idx, const double* p_val, const int32_t* s_idx, const double* s_val, const int32_t* drop,
                                   int32_t* slot, double* prior, double* grad, double* shift, int32_t* rank, int32_t* status) {
    if (!drop || !slot || !prior || !grad || !shift || !rank || !status) return locamd_fail(LOC_ERR_INVALID, "marginal prior: drop and output arrays");
    const locamd::HostBatch b{n, poses, counts, r_val, p_val, s_val, r_idx, p_idx, s_idx};
    if (int rc = validate_instances(w, b)) return rc;
    const locamd::WindowCaps& c = w->caps;
    const int bad = locamd::check_marginal_drop(c, b, drop);
    if (bad == 1) return locamd_fail(LOC_ERR_INVALID, "marginal prior: a drop slot outside its window");
    if (w->opt.has_off1) return locamd_fail(LOC_ERR_UNSUPPORTED, "marginal prior: no endpoint-1 lever arms");
    if (!locamd::translation_only(c, w->n_anchors, b, w->opt.has_pinfo) || (w->opt.has_pinfo && !w->opt.pinfo_translation))
        return locamd_fail(LOC_ERR_UNSUPPORTED, "marginal prior: translation-only batches alone (no EdgeSE3, identity rotations, zero lever arms, priors without rotation information)");
    if (bad == 2) return locamd_fail(LOC_ERR_UNSUPPORTED, "marginal prior: pose-to-pose edges join a dropped pose to more than one other pose");
    LOC_HIP(hipSetDevice(w->device));
    if (int rc = flush_anchors(w)) return rc;
    const locamd::BlockLayout L = locamd::marginal_prior_layout(c, (size_t)n);
    return staged_call(w, L, b, {{drop, 6}}, {{slot, 0}, {prior, 1}, {grad, 2}, {shift, 3}, {rank, 4}, {status, 5}}, "launch_window_marginal_prior",
                       [&](const locamd::WindowArgs& a, char* d, hipStream_t st) {
        return locamd::launch_window_marginal_prior(a, (const int32_t*)(d + L.pre[6]), (int32_t*)(d + L.pre[0]), (double*)(d + L.pre[1]), (double*)(d + L.pre[2]),
                                                    (double*)(d + L.pre[3]), (int32_t*)(d + L.pre[4]), (int32_t*)(d + L.pre[5]), st);
    });
}

int loc_window_covariance_host(loc_window* w, int64_t n, const int32_t* counts, const double* poses, const int32_t* r_idx, const double* r_val,
                               const int32_t* p_idx, const double* p_val, const int32_t* s_idx, const double* s_val, double* cov, int32_t* mask,
                               int32_t* status) {
    return loc_window_joint_covariance_host(w, n, counts, poses, r_idx, r_val, p_idx, p_val, s_idx, s_val, 0, nullptr, nullptr, cov, mask, status, nullptr);
}

// loc_window_covariance_resident is the joint call without pairs, as on the host path
int loc_window_joint_covariance_resident(loc_window* w, void* hip_stream, int32_t npair_max, const int32_t* pair_counts_host, const int32_t* pairs_host,
                                         void* cov_dev, void* mask_dev, void* status_dev, void* cross_dev) {
    if (int rc = resident_gate(w, locamd::ResidentEntry::Covariance, !cov_dev || !mask_dev || !status_dev ? 1 : 0)) return rc;
    Resident& R = w->res;
    const locamd::PairTables pt{npair_max, pair_counts_host, pairs_host};
    if (npair_max > 0)   // (the pair check reads every window's nv; a call without pairs reads no count and does not wait)
        if (int rc = refresh_mirror(w)) return rc;
    if (int rc = validate_pairs(R.n, R.counts.data(), pt, cross_dev)) return rc;
    const bool joint = npair_max > 0;
    LOC_HIP(hipSetDevice(w->device));
    loc_window::BatchSlot& S = w->slot[1];
    if (locamd::cov_stale(w->opt, w->fits, R.n, R.cov, R.env_switches)) R.cov = CovKind::Unclassified;
    if (R.cov == CovKind::Unclassified) {   // (a batch on the grouped solve path: the block of its upload, no copy-back)
        R.cov = locamd::resident_groups_covariance(w->opt, w->fits, R.n, R.groups_no_chain);
        if (R.cov != CovKind::Unclassified) R.env_switches = locamd::cov_switches(w->opt);
    }
    if (R.cov == CovKind::Unclassified && !w->opt.has_off1) {
        // first call on an upload no solve kernel classified as a chain: the uploaded tables come back once and are scanned on the host
        if (int rc = wait_resident(w)) return rc;
        const locamd::WindowCaps& c = w->caps;
        const size_t N = (size_t)R.n;
        auto len = [&](int t, size_t elem) { return N * locamd::table_bytes(c, t) / elem + 1; };
        std::vector<int32_t> counts(len(kCounts, 4)), ridx(len(locamd::kRIdx, 4)), pidx(len(locamd::kPIdx, 4)), sidx(len(locamd::kSIdx, 4));
        std::vector<double> poses(len(kPoses, 8)), rval(len(locamd::kRVal, 8)), pval(len(locamd::kPVal, 8));   // (no scan reads s_val: it stays on the device)
        void* const dst[locamd::kWindowTables] = {poses.data(), counts.data(), rval.data(), pval.data(), nullptr, ridx.data(), pidx.data(), sidx.data()};
        LOC_HIP(copy_tables(c, N, dst, uploaded_tables(w).t, hipMemcpyDeviceToHost, nullptr));
        const locamd::HostBatch b{(int64_t)N, poses.data(), counts.data(), rval.data(), pval.data(), nullptr, ridx.data(), pidx.data(), sidx.data()};
        const locamd::CovVerdict v = locamd::covariance_kind(c, w->opt, w->fits, w->n_anchors, b, locamd::PairTables{0, nullptr, nullptr}, S.cov_aux, nullptr);
        if (v.need_upload) LOC_HIP(upload_tree_sched(w, S.cov_aux, w->stream, false, v.kind == CovKind::ForestGroupsOwn));
        R.cov = v.kind;
        S.cov_list_cap = v.list_cap; S.env_blocks = v.env_blocks;
        R.env_switches = locamd::cov_switches(w->opt);
        if (v.kind == CovKind::Envelope) { R.ridx.swap(ridx); R.sidx.swap(sidx); }   // (a joint call's pairs enlarge the envelope)
    }
    if (!locamd::cov_admitted(w->opt, w->fits, R.n, R.cov)) return locamd_fail(LOC_ERR_UNSUPPORTED, "loc_window_covariance_resident" LOC_COV_UNSUPPORTED);
    const bool arrow = R.cov == CovKind::Arrow, envelope = R.cov == CovKind::Envelope;
    long long env_blocks = S.env_blocks;
    if (envelope && joint) {
        const locamd::HostBatch eb{R.n, nullptr, R.counts.data(), nullptr, nullptr, nullptr, R.ridx.data(), nullptr, R.sidx.data()};
        env_blocks = locamd::envelope_blocks_max_joint(w->caps, eb, pt);
        if (env_blocks < 0) return locamd_fail(LOC_ERR_INVALID, "joint covariance: pair tables");   // (cannot happen: validated above)
    }
    if (envelope && S.env_ws_cap < (size_t)R.n * locamd::window_envelope_covariance_workspace_doubles(w->caps, env_blocks)) {
        if (int rc = wait_resident(w)) return rc;   // (as below)
        LOC_HIP(grow_env_workspace(w, S, R.n, env_blocks));
    }
    if (arrow && S.cov_ws_cap < (size_t)R.n * locamd::window_arrow_covariance_workspace_doubles(w->caps, S.cov_list_cap)) {
        if (int rc = wait_resident(w)) return rc;   // (an earlier covariance launch may still use the workspace that is about to be replaced)
        LOC_HIP(grow_cov_workspace(w, S, R.n, S.cov_list_cap));
    }
    hipStream_t st;
    if (int rc = resident_stream(w, hip_stream, true, st)) return rc;
    locamd::CovPairs pp{nullptr, nullptr, nullptr, 0};
    const locamd::BlockLayout L = locamd::resident_pairs_layout((size_t)R.n, (size_t)npair_max);
    if (joint) {
        // the caller's arrays are read here and never after the call returns: into the page-locked copy (once the previous call's copy has
        // left it), from there to the device table in stream order below
        if (L.end > w->pairs.cap)
            if (int rc = wait_resident(w)) return rc;   // (an earlier joint launch may still read the table that is about to be replaced)
        LOC_HIP(w->pairs.reserve(L.end));
        char* h;
        LOC_HIP(w->pairs.host(h));
        std::memcpy(h + L.pre[0], pair_counts_host, L.len[0]);
        std::memcpy(h + L.pre[1], pairs_host, L.len[1]);
        pp = locamd::CovPairs{(const int32_t*)(w->pairs.d + L.pre[0]), (const int32_t*)(w->pairs.d + L.pre[1]), (double*)cross_dev, npair_max};
    }
    const int rc = resident_bracket(w, st, Timing::Covariance, [&](hipStream_t st) {
        if (joint) LOC_HIP(w->pairs.send(L.end, st));   // (after the bracket's wait: an earlier joint launch on another stream has finished reading the table)
        return (int)LOC_OK;
    }, [&](hipStream_t st) {
        const locamd::WindowArgs a = window_args(w, w->dev, R.n, nullptr, w->d_anchors, nullptr);
        return launched(launch_covariance(w, S, R.cov, env_blocks, a, (double*)cov_dev, (int32_t*)mask_dev, (int32_t*)status_dev, pp, st), "launch_window_covariance");
    });
    if (rc == LOC_OK) w->last_cov_kind = locamd::cov_public_kind(R.cov);
    return rc;
}

int loc_window_covariance_resident(loc_window* w, void* hip_stream, void* cov_dev, void* mask_dev, void* status_dev) {
    return loc_window_joint_covariance_resident(w, hip_stream, 0, nullptr, nullptr, cov_dev, mask_dev, status_dev, nullptr);
}

int loc_window_covariance_plan(const loc_window_caps* caps, int64_t n, const int32_t* counts, const int32_t* r_idx, const int32_t* s_idx,
                               int64_t* blocks_max, size_t* workspace_bytes) {
    return loc_window_joint_covariance_plan(caps, n, counts, r_idx, s_idx, 0, nullptr, nullptr, blocks_max, workspace_bytes);
}

int loc_window_joint_covariance_plan(const loc_window_caps* caps, int64_t n, const int32_t* counts, const int32_t* r_idx, const int32_t* s_idx,
                                     int32_t npair_max, const int32_t* pair_counts, const int32_t* pairs, int64_t* blocks_max, size_t* workspace_bytes) {
    if (!caps || n <= 0 || !counts || !blocks_max || !workspace_bytes) return locamd_fail(LOC_ERR_INVALID, "loc_window_covariance_plan arguments");
    if (npair_max < 0 || (npair_max > 0 && (!pair_counts || !pairs))) return locamd_fail(LOC_ERR_INVALID, "loc_window_joint_covariance_plan: pair arrays");
    if (caps->nv_max <= 0 || caps->nv_max > 4096 || caps->nr_max < 0 || caps->np_max < 0 || caps->ns_max < 0)
        return locamd_fail(LOC_ERR_UNSUPPORTED, "window capacities (1 <= nv_max <= 4096)");
    if ((caps->nr_max && !r_idx) || (caps->ns_max && !s_idx)) return locamd_fail(LOC_ERR_INVALID, "missing edge arrays");
    const locamd::WindowCaps c = to_caps(caps);
    const locamd::HostBatch b{n, nullptr, counts, nullptr, nullptr, nullptr, r_idx, nullptr, s_idx};
    const long long blocks = locamd::envelope_blocks_max_joint(c, b, locamd::PairTables{npair_max, pair_counts, pairs});
    if (blocks < 0) return locamd_fail(LOC_ERR_INVALID, "loc_window_covariance_plan: counts exceed capacities, or an edge vertex index, a pair count or a pair's pose slot is out of range");
    *blocks_max = blocks;
    *workspace_bytes = (size_t)n * locamd::window_envelope_covariance_workspace_doubles(c, blocks) * sizeof(double);
    return LOC_OK;
}

// ---- the resident slide (window_slide_kernel.hip; DESIGN.md §2, "The resident slide") ------------------------------------------------------------
// A slide's new pose and new rows as one block of pointers (the public loc_window_message_rows: host arrays for loc_window_slide_resident,
// device arrays for the other two; verdict is not used) and the capacities they were written for
struct NewRows { loc_window_message_rows p; int32_t nr, np, ns; };
static NewRows new_rows(const void* drop, const void* pose, int32_t nr, const void* rc, const void* ri, const void* rv, int32_t np, const void* pc, const void* pv,
                        int32_t ns = 0, const void* sc = nullptr, const void* si = nullptr, const void* sv = nullptr) {
    auto m = [](const void* q) { return const_cast<void*>(q); };   // (the block is the build's OUTPUT type; a slide only reads through it)
    return {{m(drop), m(pose), m(rc), m(ri), m(rv), m(pc), m(pv), m(sc), m(si), m(sv), nullptr}, nr, np, ns};
}
// the slides' argument check: the new pose and the new row arrays are all there for the capacities given
static int new_rows_missing(const NewRows& r) {
    const loc_window_message_rows& p = r.p;
    return p.new_pose && r.nr >= 0 && r.np >= 0 && r.ns >= 0 && (r.nr == 0 || (p.new_r_counts && p.new_r_idx && p.new_r_val)) && (r.np == 0 || (p.new_p_counts && p.new_p_val)) &&
           (r.ns == 0 || (p.new_s_counts && p.new_s_idx && p.new_s_val)) ? 0 : 1;
}
// the resident batch's tables and the call's new rows in a slide's argument block (SlideArgs, SlidePlainArgs)
extern "C++" {   // (a template cannot have C linkage)
template <class Args>
static void slide_tables_and_rows(const loc_window* w, const NewRows& r, Args& sa) {
    sa.counts = (int32_t*)w->dev.t[kCounts]; sa.poses = (double*)w->dev.t[kPoses]; sa.poses_in = w->d_poses_in;
    sa.r_idx = (int32_t*)w->dev.t[locamd::kRIdx]; sa.r_val = (double*)w->dev.t[locamd::kRVal];
    sa.p_idx = (int32_t*)w->dev.t[locamd::kPIdx]; sa.p_val = (double*)w->dev.t[locamd::kPVal];
    sa.drop = (const int32_t*)r.p.drop_oldest; sa.new_pose = (const double*)r.p.new_pose;
    sa.new_r_counts = (const int32_t*)r.p.new_r_counts; sa.new_r_idx = (const int32_t*)r.p.new_r_idx; sa.new_r_val = (const double*)r.p.new_r_val;
    sa.new_p_counts = (const int32_t*)r.p.new_p_counts; sa.new_p_val = (const double*)r.p.new_p_val;
    sa.nr_new_max = r.nr; sa.np_new_max = r.np; sa.B = (int)w->res.n; sa.caps = w->caps;
}
}   // extern "C++"
// the one-time allocations of a slide: the marginal pass's block for B windows (fresh: its drop table is not zeroed yet), and the table a first
// slide creates (a launch under an earlier table may still read it: that one waits)
static int slide_allocate(loc_window* w, bool densify, bool& fresh) {
    fresh = !w->d_slide_mp;
    if (fresh) LOC_HIP(hipMalloc((void**)&w->d_slide_mp, locamd::slide_marginal_layout((size_t)w->B).end));
    if (densify) {
        if (int rc = wait_resident(w)) return rc;
        if (!w->d_pinfo) LOC_HIP(hipMalloc((void**)&w->d_pinfo, (size_t)w->B * w->caps.np_max * 36 * sizeof(double)));
    }
    return LOC_OK;
}
// launch 1: the marginal of slot 0 at the solved poses, marginal_prior_kernel itself (a handle without a table: p_val's diagonals, as
// loc_window_marginal_prior_host reads them); launch 2: the re-pack — sa holds the call's inputs and outputs; admitting: the twin whose waves
// admit their own windows.  Then the handle's state but the mirror: what loc_window_upload of the slid tables, with the table set, would leave.
// rows: where the kernel reads them (the caller's device arrays, or the staging block's device half: send_bytes of it travel first); out: the
// caller's {slot, prior, rank, status}
static int slide_launches(loc_window* w, hipStream_t st, const NewRows& rows, size_t send_bytes, void* const out[4], bool densify, bool fresh, bool admitting, int32_t* admit) {
    const locamd::WindowCaps& c = w->caps;
    const int64_t n = w->res.n;
    const locamd::BlockLayout M = locamd::slide_marginal_layout((size_t)w->B);
    auto mp = [&](int piece) { return w->d_slide_mp + M.pre[piece]; };
    locamd::SlideArgs sa{};
    slide_tables_and_rows(w, rows, sa);
    sa.p_info = c.np_max > 0 ? w->d_pinfo : nullptr;
    sa.m_slot = (const int32_t*)mp(locamd::kMSlot); sa.m_prior = (const double*)mp(locamd::kMPrior); sa.m_rank = (const int32_t*)mp(locamd::kMRank); sa.m_status = (const int32_t*)mp(locamd::kMStatus);
    sa.slot = (int32_t*)out[0]; sa.prior = (double*)out[1]; sa.rank = (int32_t*)out[2]; sa.status = (int32_t*)out[3];
    const int rc = resident_bracket(w, st, Timing::Covariance, [&](hipStream_t st) {
        if (send_bytes) LOC_HIP(w->slide.send(send_bytes, st));
        if (fresh) LOC_HIP(hipMemsetAsync(mp(locamd::kMDrop), 0, M.pre[locamd::kMSlot], st));                         // the marginal pass's drop table: slot 0 of every window
        if (densify) LOC_HIP(hipMemsetAsync(w->d_pinfo, 0, (size_t)w->B * c.np_max * 36 * sizeof(double), st));     // (rows beyond the counts: zeros, not what the allocation held)
        return (int)LOC_OK;
    }, [&](hipStream_t st) {
        const locamd::WindowArgs a = window_args(w, w->dev, n, nullptr, w->d_anchors, nullptr);
        if (int rc = launched(locamd::launch_window_marginal_prior(a, (const int32_t*)mp(locamd::kMDrop), (int32_t*)mp(locamd::kMSlot), (double*)mp(locamd::kMPrior), (double*)mp(locamd::kMGrad),
                                                                   (double*)mp(locamd::kMShift), (int32_t*)mp(locamd::kMRank), (int32_t*)mp(locamd::kMStatus), st), "launch_window_marginal_prior")) return rc;
        return launched(admitting ? locamd::launch_window_slide_dev(sa, w->n_anchors, admit, densify, st) : locamd::launch_window_slide(sa, densify, st), "launch_window_slide");
    });
    if (rc) return rc;
    if (densify) { w->opt.has_pinfo = true; w->opt.pinfo_translation = true; w->n_pinfo = n; }
    w->res.skip = locamd::structured_pinfo(w->opt);
    w->res.cov = CovKind::Chain3;   // (loc_window_upload's verdict for this topology; a call the switches do not admit classifies it again)
    return LOC_OK;
}

int loc_window_slide_resident(loc_window* w, void* hip_stream, const int32_t* drop_oldest, const double* new_pose,
                              int32_t nr_new_max, const int32_t* new_r_counts, const int32_t* new_r_idx, const double* new_r_val,
                              int32_t np_new_max, const int32_t* new_p_counts, const double* new_p_val,
                              void* slot_dev, void* prior_dev, void* rank_dev, void* status_dev) {
    const NewRows given = new_rows(drop_oldest, new_pose, nr_new_max, new_r_counts, new_r_idx, new_r_val, np_new_max, new_p_counts, new_p_val);
    if (int rc = resident_gate(w, locamd::ResidentEntry::SlideHost, new_rows_missing(given))) return rc;
    if (int rc = refresh_mirror(w)) return rc;   // (the two entries may alternate on one handle)
    const locamd::WindowCaps& c = w->caps;
    Resident& R = w->res;
    const int64_t n = R.n;
    const size_t N = (size_t)n;
    const locamd::SlideRows rows{drop_oldest, nr_new_max, new_r_counts, new_r_idx, np_new_max, new_p_counts};
    static const char* const kWhat[] = {nullptr, "loc_window_slide_resident: a window without poses", "loc_window_slide_resident: a new count outside [0, *_new_max]",
                                        "loc_window_slide_resident: a new range index (the new slot, the slot before it or an anchor; rows in the order of their later pose)",
                                        "loc_window_slide_resident: the slid window exceeds nv_max", "loc_window_slide_resident: the slid window exceeds nr_max",
                                        "loc_window_slide_resident: the slid window exceeds np_max"};
    if (const int bad = locamd::slide_indices(c, w->n_anchors, n, R.counts.data(), R.mir_ridx.data(), R.mir_pidx.data(), rows, false).bad)
        return locamd_fail(LOC_ERR_INVALID, kWhat[bad]);
    if (!locamd::slide_rows_translation_only(n, rows, new_pose, new_r_val, new_p_val))
        return locamd_fail(LOC_ERR_UNSUPPORTED, "loc_window_slide_resident: a new row is not translation-only (identity rotations, zero lever arms, no rotation information)");
    hipStream_t st;
    if (int rc = resident_stream(w, hip_stream, true, st)) return rc;
    const locamd::BlockLayout L = locamd::slide_inputs_layout(N, (size_t)nr_new_max, (size_t)np_new_max);
    if (L.end > w->slide.cap)
        if (int rc = wait_resident(w)) return rc;   // (an earlier slide may still read the block that is about to be replaced)
    LOC_HIP(w->slide.reserve(L.end));
    const bool densify = !w->opt.has_pinfo && c.np_max > 0;
    bool fresh;
    if (int rc = slide_allocate(w, densify, fresh)) return rc;
    char* h;
    LOC_HIP(w->slide.host(h));
    {   // the caller's arrays are read here and never after the call returns
        int32_t* hd = (int32_t*)(h + L.pre[0]);
        if (drop_oldest) std::memcpy(hd, drop_oldest, L.len[0]);
        else for (size_t i = 0; i < N; ++i) hd[i] = 1;
        const void* const src[7] = {nullptr, new_r_counts, new_p_counts, new_r_idx, new_pose, new_r_val, new_p_val};
        for (int k = 1; k < 7; ++k)
            if (L.len[k] && src[k]) std::memcpy(h + L.pre[k], src[k], L.len[k]);
    }
    const char* d = w->slide.d;
    const NewRows staged = new_rows(d + L.pre[0], d + L.pre[4], nr_new_max, d + L.pre[1], d + L.pre[3], d + L.pre[5], np_new_max, d + L.pre[2], d + L.pre[6]);
    void* const out[4] = {slot_dev, prior_dev, rank_dev, status_dev};
    if (int rc = slide_launches(w, st, staged, L.end, out, densify, fresh, false, nullptr)) return rc;
    R.min_anchors = locamd::slide_indices(c, w->n_anchors, n, R.counts.data(), R.mir_ridx.data(), R.mir_pidx.data(), rows, true).max_anchor;
    return LOC_OK;
}

// the twin that takes the call's per-window inputs from DEVICE arrays: no pass over per-window data on the host, no copy, no synchronisation
// (but the one-time allocations slide_allocate makes); each wave admits its own window (slide_admit.h) and the host's mirror goes stale.  First
// its internal form, past the gate, on a stream resident_stream chose: loc_window_push_messages_resident_dev enters here
static int slide_carry_dev(loc_window* w, hipStream_t st, const NewRows& rows, void* const out[4], void* admit_dev) {
    const bool densify = !w->opt.has_pinfo && w->caps.np_max > 0;
    bool fresh;
    if (int rc = slide_allocate(w, densify, fresh)) return rc;
    if (int rc = slide_launches(w, st, rows, 0, out, densify, fresh, true, (int32_t*)admit_dev)) return rc;
    w->res.mirror_stale = true;   // (refresh_mirror: the next reader of the mirror fetches it)
    return LOC_OK;
}
int loc_window_slide_resident_dev(loc_window* w, void* hip_stream, const void* drop_oldest_dev, const void* new_pose_dev,
                                  int32_t nr_new_max, const void* new_r_counts_dev, const void* new_r_idx_dev, const void* new_r_val_dev,
                                  int32_t np_new_max, const void* new_p_counts_dev, const void* new_p_val_dev,
                                  void* slot_dev, void* prior_dev, void* rank_dev, void* status_dev, void* admit_dev) {
    const NewRows rows = new_rows(drop_oldest_dev, new_pose_dev, nr_new_max, new_r_counts_dev, new_r_idx_dev, new_r_val_dev, np_new_max, new_p_counts_dev, new_p_val_dev);
    if (int rc = resident_gate(w, locamd::ResidentEntry::SlideDev, new_rows_missing(rows))) return rc;
    hipStream_t st;
    if (int rc = resident_stream(w, hip_stream, true, st)) return rc;
    void* const out[4] = {slot_dev, prior_dev, rank_dev, status_dev};
    return slide_carry_dev(w, st, rows, out, admit_dev);
}

// the plain drop for the ordered 6-DoF chain verdicts (window_slide_plain_kernel.hip; DESIGN.md §2, "The plain drop for 6-DoF chain windows"): what
// Robot::new_vertex does with its oldest pose (robot.cpp:92-98).  One launch, nothing carried, no table; device arrays, no host pass, no copy,
// no synchronisation and no allocation; each wave admits its own window (slide_plain_admit.h) and the host's mirror goes stale.  First the
// internal form, as slide_carry_dev
static int slide_plain_dev(loc_window* w, hipStream_t st, const NewRows& rows, void* status_dev, void* admit_dev) {
    const int topology = resident_topology(w);
    locamd::SlidePlainArgs sa{};
    slide_tables_and_rows(w, rows, sa);
    sa.s_idx = (int32_t*)w->dev.t[locamd::kSIdx]; sa.s_val = (double*)w->dev.t[locamd::kSVal];
    sa.new_s_counts = (const int32_t*)rows.p.new_s_counts; sa.new_s_idx = (const int32_t*)rows.p.new_s_idx; sa.new_s_val = (const double*)rows.p.new_s_val;
    sa.status = (int32_t*)status_dev; sa.admit = (int32_t*)admit_dev; sa.ns_new_max = rows.ns; sa.n_anchors = w->n_anchors;
    sa.pair_rule = topology == LOC_WINDOW_KERNEL_WAVE6 ? locamd::kSlidePairsWave6 : topology == LOC_WINDOW_KERNEL_WAVE6S ? locamd::kSlidePairsWave6S : locamd::kSlidePairsNone;
    if (int rc = resident_bracket(w, st, Timing::Covariance, nothing_staged, [&](hipStream_t st) { return launched(locamd::launch_window_slide_plain(sa, st), "launch_window_slide_plain"); }))
        return rc;
    w->res.cov = CovKind::Chain6;     // (loc_window_upload's verdict for these topologies; a batch the envelope pass held is classified again)
    w->res.mirror_stale = true;       // (refresh_mirror: the next reader of the mirror fetches it)
    return LOC_OK;
}
int loc_window_slide_plain_resident_dev(loc_window* w, void* hip_stream, const void* drop_oldest_dev, const void* new_pose_dev,
                                        int32_t nr_new_max, const void* new_r_counts_dev, const void* new_r_idx_dev, const void* new_r_val_dev,
                                        int32_t np_new_max, const void* new_p_counts_dev, const void* new_p_val_dev,
                                        int32_t ns_new_max, const void* new_s_counts_dev, const void* new_s_idx_dev, const void* new_s_val_dev,
                                        void* status_dev, void* admit_dev) {
    const NewRows rows = new_rows(drop_oldest_dev, new_pose_dev, nr_new_max, new_r_counts_dev, new_r_idx_dev, new_r_val_dev, np_new_max, new_p_counts_dev, new_p_val_dev,
                                  ns_new_max, new_s_counts_dev, new_s_idx_dev, new_s_val_dev);
    if (int rc = resident_gate(w, locamd::ResidentEntry::SlidePlain, new_rows_missing(rows))) return rc;
    hipStream_t st;
    if (int rc = resident_stream(w, hip_stream, true, st)) return rc;
    return slide_plain_dev(w, st, rows, status_dev, admit_dev);
}

// ---- rows from raw messages (window_message_kernel.hip, message_rows.h; DESIGN.md §2, "Rows from raw messages") ----------------------------------
// Localization::addRangeEdge (localization.cpp:297-376), Robot::new_vertex (robot.cpp:75-110), addImuEdge (:499-535), addLidarEdge (:462-496) and
// addTwistEdge (:438-459, :560-605) for a resident batch: the configuration those read (:72-78, :111-123), per handle
int loc_window_set_message_config(loc_window* w, const loc_window_message_config* cfg, int32_t n_antenna, const double* antenna_xyz_host) {
    if (!w || !cfg) return locamd_fail(LOC_ERR_INVALID, "loc_window_set_message_config: null");
    if (cfg->trajectory_length < 1 || cfg->trajectory_length > w->caps.nv_max)
        return locamd_fail(LOC_ERR_INVALID, "loc_window_set_message_config: trajectory_length must be in [1, nv_max]");
    if (!(cfg->maximum_velocity == cfg->maximum_velocity) || !(cfg->distance_outlier == cfg->distance_outlier))
        return locamd_fail(LOC_ERR_INVALID, "loc_window_set_message_config: maximum_velocity and distance_outlier must be numbers");
    if (n_antenna < 0 || (n_antenna > 0 && !antenna_xyz_host)) return locamd_fail(LOC_ERR_INVALID, "loc_window_set_message_config: the antenna table");
    LOC_HIP(hipSetDevice(w->device));
    if (int rc = wait_resident(w)) return rc;   // a resident launch may still be reading the table
    if (n_antenna > w->antenna_cap) {
        double* p = nullptr;
        LOC_HIP(hipMalloc((void**)&p, (size_t)n_antenna * 3 * sizeof(double)));
        if (w->d_antenna) (void)hipFree(w->d_antenna);
        w->d_antenna = p;
        w->antenna_cap = n_antenna;
    }
    if (n_antenna > 0) LOC_HIP(hipMemcpy(w->d_antenna, antenna_xyz_host, (size_t)n_antenna * 3 * sizeof(double), hipMemcpyHostToDevice));
    if (!w->d_msg_rows) LOC_HIP(hipMalloc((void**)&w->d_msg_rows, locamd::message_rows_layout((size_t)w->B).end));
    w->n_antenna = n_antenna;
    w->msg_cfg = *cfg;
    w->msg_set = true;
    return LOC_OK;
}
// the argument checks both entries share, in their order (loc_window_message_rows_dev has a fourth: its output arrays)
static int message_args_failed(int32_t kinds_mask, const loc_window_messages* m) {
    if ((kinds_mask & ~locamd::kMsgAllKinds) != 0) return 1;
    if (!m || !m->kind || !m->dt) return 2;
    if (((kinds_mask & LOC_MSG_RANGE) && (!m->anchor || !m->antenna || !m->distance || !m->distance_err)) || ((kinds_mask & LOC_MSG_IMU) && !m->imu) ||
        ((kinds_mask & LOC_MSG_LIDAR) && !m->lidar_z) || ((kinds_mask & LOC_MSG_TWIST) && !m->twist))
        return 3;
    return 0;
}
// the build launch, in its bracket; timing: the covariance events around it, or none
static int message_launch(loc_window* w, hipStream_t st, int32_t kinds_mask, const loc_window_messages* m, const loc_window_message_rows& o, Timing timing) {
    locamd::MessageArgs a{};
    a.counts = (const int32_t*)w->dev.t[kCounts]; a.poses = (const double*)w->dev.t[kPoses];
    a.anchors = w->d_anchors; a.antenna_xyz = w->d_antenna; a.n_anchors = w->n_anchors; a.n_antenna = w->n_antenna;
    a.trajectory_length = w->msg_cfg.trajectory_length; a.maximum_velocity = w->msg_cfg.maximum_velocity; a.distance_outlier = w->msg_cfg.distance_outlier;
    a.kinds_mask = kinds_mask;
    a.kind = (const int32_t*)m->kind; a.dt = (const double*)m->dt;
    a.anchor = (const int32_t*)m->anchor; a.antenna = (const int32_t*)m->antenna; a.distance = (const float*)m->distance; a.distance_err = (const float*)m->distance_err;
    a.imu = (const double*)m->imu; a.lidar_z = (const double*)m->lidar_z; a.twist = (const double*)m->twist;
    a.drop_oldest = (int32_t*)o.drop_oldest; a.new_pose = (double*)o.new_pose;
    a.new_r_counts = (int32_t*)o.new_r_counts; a.new_r_idx = (int32_t*)o.new_r_idx; a.new_r_val = (double*)o.new_r_val;
    a.new_p_counts = (int32_t*)o.new_p_counts; a.new_p_val = (double*)o.new_p_val;
    a.new_s_counts = (int32_t*)o.new_s_counts; a.new_s_idx = (int32_t*)o.new_s_idx; a.new_s_val = (double*)o.new_s_val;
    a.verdict = (int32_t*)o.verdict;
    a.B = (int)w->res.n; a.nv_max = w->caps.nv_max;
    return resident_bracket(w, st, timing, nothing_staged, [&](hipStream_t st) { return launched(locamd::launch_window_message_rows(a, st), "launch_window_message_rows"); });
}

// build only (the rows of localization.cpp:297-376, :438-535 and :560-605 at robot.cpp:90's estimate), into the caller's device arrays: every resident verdict (only counts and poses are read); no host pass, no copy, no
// synchronisation, no allocation
int loc_window_message_rows_dev(loc_window* w, void* hip_stream, int32_t kinds_mask, const loc_window_messages* msgs, const loc_window_message_rows* out) {
    int bad = message_args_failed(kinds_mask, msgs);
    if (!bad && (!out || !out->drop_oldest || !out->new_pose || !out->new_r_counts || !out->new_r_idx || !out->new_r_val || !out->new_p_counts || !out->new_p_val ||
                 !out->new_s_counts || !out->new_s_idx || !out->new_s_val))
        bad = 4;
    if (int rc = resident_gate(w, locamd::ResidentEntry::MessageRows, bad)) return rc;
    hipStream_t st;
    if (int rc = resident_stream(w, hip_stream, true, st)) return rc;
    return message_launch(w, st, kinds_mask, msgs, *out, Timing::Covariance);
}

// build into the handle's block (untimed), then the slide the resident verdict calls for (robot.cpp:92-98: drop-oldest) in a bracket of its own on
// the same stream.  Both slides' host refusals are the rule's, taken BEFORE the build, so a refusal launches nothing
int loc_window_push_messages_resident_dev(loc_window* w, void* hip_stream, int32_t kinds_mask, const loc_window_messages* msgs,
                                          void* verdict_dev, void* status_dev, void* admit_dev) {
    if (int rc = resident_gate(w, locamd::ResidentEntry::PushMessages, message_args_failed(kinds_mask, msgs))) return rc;
    hipStream_t st;
    if (int rc = resident_stream(w, hip_stream, true, st)) return rc;
    const locamd::MessageRowsLayout L = locamd::message_rows_layout((size_t)w->B);
    auto at = [&](int piece) { return (void*)(w->d_msg_rows + L.off[piece]); };
    const loc_window_message_rows o{at(locamd::kGDrop), at(locamd::kGPose), at(locamd::kGRCounts), at(locamd::kGRIdx), at(locamd::kGRVal), at(locamd::kGPCounts),
                                    at(locamd::kGPVal), at(locamd::kGSCounts), at(locamd::kGSIdx), at(locamd::kGSVal), verdict_dev ? verdict_dev : at(locamd::kGVerdict)};
    if (int rc = message_launch(w, st, kinds_mask, msgs, o, Timing::None)) return rc;
    if (resident_topology(w) != LOC_WINDOW_KERNEL_CHAIN3) return slide_plain_dev(w, st, NewRows{o, LOC_MSG_NR_NEW, LOC_MSG_NP_NEW, LOC_MSG_NS_NEW}, status_dev, admit_dev);
    void* const out[4] = {nullptr, nullptr, nullptr, status_dev};
    return slide_carry_dev(w, st, NewRows{o, LOC_MSG_NR_NEW, LOC_MSG_NP_NEW, 0}, out, admit_dev);
}

// ---- the per-edge chi2 audit and the outlier-range removal (edge_audit_kernel.hip; DESIGN.md §2, "Edge audit and outlier removal") ----------------
// stateless and synchronous (staged_call: the resident batch's arrays and the host path's cached verdict are not touched); every structure
// and every handle state, so there is no dispatch and no UNSUPPORTED case
int loc_window_edge_chi2_host(loc_window* w, int64_t n, const int32_t* counts, const double* poses, const int32_t* r_idx, const double* r_val,
                              const int32_t* p_idx, const double* p_val, const int32_t* s_idx, const double* s_val,
                              double* r_chi2, double* p_chi2, double* s_chi2, double* total, int32_t* active) {
    const locamd::HostBatch b{n, poses, counts, r_val, p_val, s_val, r_idx, p_idx, s_idx};
    if (int rc = validate_instances(w, b)) return rc;
    LOC_HIP(hipSetDevice(w->device));
    if (int rc = flush_anchors(w)) return rc;
    const locamd::BlockLayout L = locamd::edge_audit_layout(w->caps, (size_t)n);
    return staged_call(w, L, b, {}, {{r_chi2, 0}, {p_chi2, 1}, {s_chi2, 2}, {total, 3}, {active, 4}}, "launch_window_edge_audit",
                       [&](const locamd::WindowArgs& a0, char* d, hipStream_t st) {
        locamd::WindowArgs a = a0;
        a.r_off1 = w->opt.has_off1 ? w->d_roff1 : nullptr;   // (window_args hands the lever arms of endpoint 1 to the solves alone)
        const locamd::EdgeAudit x{(double*)(d + L.pre[0]), (double*)(d + L.pre[1]), (double*)(d + L.pre[2]), (double*)(d + L.pre[3]), (int32_t*)(d + L.pre[4]),
                                  nullptr, 0.0, 0, nullptr, nullptr};
        return locamd::launch_window_edge_audit(a, x, st);
    });
}

// the two resident entries' launch, in the bracket (resident_launch); nothing is read on the host, nothing synchronises, the mirror stays as it is
static int resident_audit_launch(loc_window* w, void* hip_stream, const locamd::EdgeAudit& x) {
    return resident_launch(w, hip_stream, Timing::Covariance, true, [&](hipStream_t st) {
        locamd::WindowArgs a = window_args(w, w->dev, w->res.n, nullptr, w->d_anchors, nullptr);
        a.r_off1 = w->opt.has_off1 ? w->d_roff1 : nullptr;
        return launched(locamd::launch_window_edge_audit(a, x, st), "launch_window_edge_audit");
    });
}

int loc_window_edge_chi2_resident(loc_window* w, void* hip_stream, void* r_chi2_dev, void* p_chi2_dev, void* s_chi2_dev, void* total_dev, void* active_dev) {
    if (int rc = resident_gate(w, locamd::ResidentEntry::EdgeChi2)) return rc;
    return resident_audit_launch(w, hip_stream, locamd::EdgeAudit{(double*)r_chi2_dev, (double*)p_chi2_dev, (double*)s_chi2_dev, (double*)total_dev, (int32_t*)active_dev, nullptr, 0.0, 0, nullptr, nullptr});
}

int loc_window_prune_resident(loc_window* w, void* hip_stream, double chi2_max, int32_t min_edges, void* removed_dev, void* n_removed_dev) {
    if (int rc = resident_gate(w, locamd::ResidentEntry::Prune, !(chi2_max >= 0.0) || min_edges < 0 ? 1 : 0)) return rc;
    return resident_audit_launch(w, hip_stream, locamd::EdgeAudit{nullptr, nullptr, nullptr, nullptr, nullptr, (double*)w->dev.t[locamd::kRVal], chi2_max, min_edges,
                                                                  (int32_t*)removed_dev, (int32_t*)n_removed_dev});
}

// ---- the publish step and the path of the resident batch (window_publish_kernel.hip; DESIGN.md §2, "Publish and path records of a resident
// batch"): Localization::publish() (localization.cpp:195-226), Robot::vertices2path() (robot.cpp:61-72), the destructor's tail (:708-717) ----
// Both entries: their argument checks in the rule's order, then one launch in the bracket WITHOUT the anchor table's flush (resident_launch).
// Nothing is read on the host, nothing synchronises, the mirror stays as it is.  Only counts, poses and result are read: every structural
// verdict and every handle state, no anchors, no table of full matrices
static bool trajectory_length_bad(const loc_window* w, int32_t trajectory_length) { return w && (trajectory_length < 1 || trajectory_length > w->caps.nv_max); }

int loc_window_publish_resident(loc_window* w, void* hip_stream, double minimum_optimize_error, int32_t trajectory_length,
                                void* flags_dev, void* realtime_dev, void* optimized_dev, void* chi2_dev, void* n_published_dev) {
    const int bad = minimum_optimize_error != minimum_optimize_error ? 1 : !flags_dev ? 2 : trajectory_length_bad(w, trajectory_length) ? 3 : 0;
    if (int rc = resident_gate(w, locamd::ResidentEntry::Publish, bad)) return rc;
    return resident_launch(w, hip_stream, Timing::Covariance, false, [&](hipStream_t st) {
        const locamd::PublishArgs a{(const int32_t*)w->dev.t[kCounts], (const double*)w->dev.t[kPoses], w->d_result, minimum_optimize_error, trajectory_length,
                                    (int32_t*)flags_dev, (double*)realtime_dev, (double*)optimized_dev, (double*)chi2_dev, (int32_t*)n_published_dev,
                                    w->res.n, w->caps.nv_max};
        return launched(locamd::launch_window_publish(a, st), "launch_window_publish");
    });
}

int loc_window_path_resident(loc_window* w, void* hip_stream, int32_t trajectory_length, int32_t first, int32_t count, void* path_dev, void* present_dev) {
    const int bad = !path_dev || !present_dev ? 1 : first < 0 || count < 1 || (int64_t)first + count > trajectory_length ? 2 : trajectory_length_bad(w, trajectory_length) ? 3 : 0;
    if (int rc = resident_gate(w, locamd::ResidentEntry::Path, bad)) return rc;
    return resident_launch(w, hip_stream, Timing::Covariance, false, [&](hipStream_t st) {
        const locamd::PathArgs a{(const int32_t*)w->dev.t[kCounts], (const double*)w->dev.t[kPoses], trajectory_length, first, count,
                                 (double*)path_dev, (int32_t*)present_dev, w->res.n, w->caps.nv_max};
        return launched(locamd::launch_window_path(a, st), "launch_window_path");
    });
}

int loc_window_download_tables(loc_window* w, int32_t* counts, double* poses, int32_t* r_idx, double* r_val, int32_t* p_idx, double* p_val,
                               int32_t* s_idx, double* s_val, double* pinfo) {
    if (int rc = resident_gate(w, locamd::ResidentEntry::DownloadTables, w && pinfo && !w->opt.has_pinfo ? 1 : 0)) return rc;
    LOC_HIP(hipSetDevice(w->device));
    if (int rc = wait_resident(w)) return rc;
    const locamd::WindowCaps& c = w->caps;
    const size_t N = (size_t)w->res.n;
    void* dst[locamd::kWindowTables] = {nullptr};
    dst[kPoses] = poses; dst[kCounts] = counts; dst[locamd::kRVal] = r_val; dst[locamd::kPVal] = p_val; dst[locamd::kSVal] = s_val;
    dst[locamd::kRIdx] = r_idx; dst[locamd::kPIdx] = p_idx; dst[locamd::kSIdx] = s_idx;
    LOC_HIP(copy_tables(c, N, dst, uploaded_tables(w).t, hipMemcpyDeviceToHost, nullptr));
    const size_t n_info = std::min(N, (size_t)w->n_pinfo);
    if (pinfo) LOC_HIP(hipMemcpy(pinfo, w->d_pinfo, n_info * c.np_max * 36 * sizeof(double), hipMemcpyDeviceToHost));
    return LOC_OK;
}

int loc_window_last_covariance_ms(loc_window* w, double* ms) {
    if (!w || !ms) return locamd_fail(LOC_ERR_INVALID, "null");
    if (w->cov_pending) {
        LOC_HIP(hipSetDevice(w->device));
        LOC_HIP(hipEventSynchronize(w->cov_ev1));
        float t = 0;
        LOC_HIP(hipEventElapsedTime(&t, w->cov_ev0, w->cov_ev1));
        w->cov_ms = t;
        w->cov_pending = false;
    }
    *ms = w->cov_ms;
    return LOC_OK;
}

}  // extern "C"
