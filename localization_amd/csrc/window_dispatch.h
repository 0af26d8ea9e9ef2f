// Which solve kernel and which covariance pass a batch of windows takes: the rules, free of any handle and HIP state (window_dispatch.cpp
// compiles with a plain host compiler, as window_structure.cpp does; tests/host/window_dispatch_driver.cpp runs the rules on the CPU).
// capi_window.cpp keeps the switches and the capacity facts in its handle and asks here; a new kernel or covariance pass is registered
// in pick_kernel / batch_topology or CovKind / covariance_kind / cov_admitted, and gets its launch in capi_window.cpp.  What a resident entry
// refuses by the handle's state alone, in which order and with which words, is resident_refusal: a new resident entry is registered in
// ResidentEntry and gets its line there.
#pragma once
#include "window_admit.h"
#include "window_structure.h"

namespace locamd {

// kernel-selection switches: the environment is read ONCE, by loc_window_create (loc_window_set_option and the setters change them afterwards)
struct DispatchOpts {
    long long env_chain_min = 12288;   // LOCAMD_CHAIN_MIN_BATCH, or the default
    bool env_chain_min_set = false;
    int arrow3 = -1;                   // LOCAMD_ARROW3: -1 default (windows of more than 64 poses), 0 never, 1 whenever the batch qualifies
    int tree = -1;                     // LOCAMD_TREE: -1 default, 0 never, 2 the lane-per-window variant
    bool wave3 = true, wave6 = true, chain3 = true, zero_copy = true, topology_cache = true;
    bool cov_general = false;          // "covariance_general" 1: whatever the three structured covariance passes decline goes to envelope_covariance_kernel.hip
    bool kernel_events = true;         // "kernel_events" 0: no HIP events around the launch of a zero-copy solve (loc_window_last_kernel_ms then reports launch-to-completion on the host clock)
    long long chain_min = -1;          // smallest batch that takes a lane-per-window kernel (-1: the default / LOCAMD_CHAIN_MIN_BATCH)
    bool natural_order = false;        // loc_window_set_ordering
    bool has_off1 = false;             // lever arms of endpoint 1 are set (loc_window_set_endpoint1_offsets)
    bool has_pinfo = false;            // full information matrices of the priors are set (loc_window_set_prior_information)
    bool pinfo_translation = false;    // ... and none of them has rotation rows or columns (prior_information_translation_only, taken once by the setter)
    bool pinfo_structured = false;     // "prior_information_structured" 1: a translation-only table on a translation-only chain is served by
                                       // wave3_lm_kernel<JAC, true> and the chain 3x3 covariance pass (structured_pinfo); 0: the general kernel, the envelope pass
    bool forest_groups = false;        // "forest_groups" 1: a batch of forest windows whose topologies DIFFER (build_tree_sched declines it) is grouped by topology
                                       // (build_tree_groups) and solved by tree_wave_kernel<JAC, TreeGroups>; 0: such a batch is LOC_WINDOW_KERNEL_GENERAL
    bool forest_groups_cov = false;    // "forest_groups_covariance" 1 (with "forest_groups" 1): the covariances of such a batch are served by
                                       // forest_covariance_kernel<JAC, JOINT, TreeGroups> on the groups' schedules; 0: the envelope pass under "covariance_general", else unsupported
    bool upload_dev_structures = false; // "upload_dev_structures" 1: loc_window_upload_dev takes batch_topology's arrowhead and forest tests on the device
                                       // (window_structure_kernel.hip) for a batch that is no chain; 0: such a batch is LOC_WINDOW_KERNEL_GENERAL
    bool upload_dev_forest_groups = false; // "upload_dev_forest_groups" 1 (with "upload_dev_structures" and "forest_groups" 1): loc_window_upload_dev groups a mixed
                                       // forest batch by topology on the device (window_groups_kernel.hip) and leaves it on the grouped kernel; 0: the general kernel
    int upload_dev_groups_hash_bits = 64;  // "upload_dev_groups_hash_bits": a test seam — that pass's candidate hash keeps this many low bits (fewer: collisions, the same answer)
};

// what depends on the handle's capacities alone: the kernels' LDS needs against their limits (window_layouts.h), taken once by loc_window_create
struct DispatchFits {
    bool wave6 = false;          // nv_max <= 64 and wave6_lm_kernel's LDS
    bool wave6_se3 = false;      // nv_max <= 63, ns_max <= 64 and wave6_lm_kernel<JAC, true>'s LDS
    bool wave3 = false;          // nv_max <= 64 and wave3_lm_kernel's LDS
    bool wave3_pinfo = false;    // the same with the prior records of wave3_lm_kernel<JAC, true> (a dense 3x3 block per prior)
    bool cov_chain = false, cov_arrow = false, cov_envelope = false;   // the chain (6x6) / arrowhead / envelope covariance pass within 160 KiB
    int nv_max = 0;
};
DispatchFits dispatch_fits(const WindowCaps& c);

// the covariance pass of a batch
enum class CovKind : int {
    Unclassified = -1,   // the first covariance call classifies the batch
    None = 0,            // not covered (LOC_ERR_UNSUPPORTED)
    Chain3, Chain6,      // covariance_kernel.hip with 3x3 (translation-only batches) / 6x6 blocks
    Forest, ForestOwn,   // forest_covariance_kernel.hip on the solve's schedule / on the schedule the covariance pass built itself
    Arrow,               // arrow_covariance_kernel.hip
    Envelope,            // envelope_covariance_kernel.hip (option "covariance_general")
    ForestGroups, ForestGroupsOwn   // forest_covariance_groups_kernel.hip (options "forest_groups" + "forest_groups_covariance") on the resident solve's groups
                                    // block / on the block the covariance pass built itself
};

// the handle's table of full information matrices is one the 3 x 3 kernels take: option "prior_information_structured", a translation-only table,
// no endpoint-1 lever arms.  While it holds, translation_only is asked with the prior diagonals skipped (p_val[12..17] is not read under a table)
bool structured_pinfo(const DispatchOpts& o);
long long effective_chain_min(const DispatchOpts& o);
long long tree_min_batch(const DispatchOpts& o);
bool arrow3_wanted(const DispatchOpts& o, const DispatchFits& f);
// The grouped forest's rule short of the structure test, stated once for the solve (batch_topology) and the covariances
// (structured_covariance_kind): option "forest_groups", option "tree" neither 0 nor 2 (tree_lm_kernel has no per-window-schedule twin), a batch of
// at least tree_min_batch windows, a handle of windows of <= 64 poses, nothing that only the general kernel evaluates.  build_tree_groups decides the rest.
bool forest_groups_wanted(const DispatchOpts& o, const WindowCaps& c, int64_t n);
// the LOC_WINDOW_COV_* of a pass (loc_window_last_covariance_kind): Forest / ForestOwn and ForestGroups / ForestGroupsOwn are one pass each
int cov_public_kind(CovKind kind);
// A resident batch whose covariance verdict is open, and which loc_window_upload put on the grouped solve path (its groups block is on the device)
// without finding a chain in any edge order (groups_no_chain), is ForestGroups under the switches as they are now — no copy-back, no scan; else Unclassified
CovKind resident_groups_covariance(const DispatchOpts& o, const DispatchFits& f, int64_t n, bool groups_no_chain);
// the switches the three structured covariance tests read besides the batch itself, as one word (option "arrow3", option "tree", the forest threshold, has_pinfo,
// option "prior_information_structured", the table's translation-only verdict; options "forest_groups" and "forest_groups_covariance" both 1)
long long cov_switches(const DispatchOpts& o);
// the kernel a batch of n windows of that structure (batch_topology's verdict) takes NOW (threshold, ordering override, the options)
int pick_kernel(const DispatchOpts& o, const DispatchFits& f, int64_t n, int topology);
// may the resident batch of n windows with verdict `kind` be served now
bool cov_admitted(const DispatchOpts& o, const DispatchFits& f, int64_t n, CovKind kind);
// is that verdict out of date: the batch is classified again under the switches as they are now.  env_switches: cov_switches() when it was classified
bool cov_stale(const DispatchOpts& o, const DispatchFits& f, int64_t n, CovKind kind, long long env_switches);

// structural verdict of the last host-path batch, keyed on a hash of (n, counts, index tables): a caller that replays one graph
// with new measurements (the node's window between two slides, a Monte-Carlo batch) skips the chain / forest / arrowhead tests
struct TopoCache {
    bool valid = false;
    unsigned long long key = 0;
    int64_t n = 0;
    bool chain = false, single_pairs = false, se3_pairs = false, tree_ok = false, tree_tried = false;
    bool groups_ok = false, groups_tried = false;   // build_tree_groups' verdict (option "forest_groups"): a refusal is remembered as well
};
struct Topology { int kind; bool cached; };   // LOC_WINDOW_KERNEL_* by structure; the verdict came from the cache
Topology batch_topology(const WindowCaps& c, const DispatchOpts& o, const DispatchFits& f, int n_anchors, const HostBatch& b, WinAux& aux, TopoCache* tc);
// The chain family of that verdict from a batch's reduced flags (window_admit.h: what window_admit_kernel.hip leaves of a batch uploaded from
// device arrays, loc_window_upload_dev): batch_topology's `if (chain)` block restated — LOC_WINDOW_KERNEL_CHAIN3 (structured_pinfo(o) chooses
// which of the two translation-only flags is read), _WAVE6, _WAVE6S, _CHAIN.  Every other batch is _GENERAL here: the arrowhead and forest
// verdicts are taken by loc_window_upload_dev itself under option "upload_dev_structures" (capi_window.cpp: dev_structures — the two tests
// that follow the chain block in batch_topology, in its order and under its conditions, on the device); without the option a forest- or
// arrowhead-shaped batch uploaded from device arrays solves on the general kernel, correctly.
int topology_from_flags(const DispatchOpts& o, const DispatchFits& f, const WindowBatchFlags& b);
// what only the general kernel evaluates (lever arms on endpoint 1, full information matrices): build_tree_sched's has_off1 argument
bool general_only(const DispatchOpts& o);

// the structure the host path's own forest schedule (its cov_aux) was built for, device copy included
struct SchedKey {
    bool valid = false;
    unsigned long long key = 0;
    int64_t n = 0;
    CovKind kind = CovKind::None;   // what the tables of that structure are: ForestOwn (a one-topology schedule) or ForestGroupsOwn (a groups block)
};
// need_upload: `own` holds a new forest schedule (ForestOwn) or groups block (ForestGroupsOwn) for the caller to send to the device; list_cap: the arrowhead pass's list size;
// env_blocks: the batch's largest envelope
struct CovVerdict { CovKind kind; bool need_upload; int list_cap; long long env_blocks; };
CovVerdict covariance_kind(const WindowCaps& c, const DispatchOpts& o, const DispatchFits& f, int n_anchors, const HostBatch& b, const PairTables& pt,
                           WinAux& own, SchedKey* keyed);

// ---- what every resident entry refuses by the handle's state, in which order and with which words ------------------------------------------
enum class ResidentEntry : int { Solve, Download, Covariance, SlideHost, SlideDev, SlidePlain, MessageRows, PushMessages, EdgeChi2, Prune, Publish, Path, DownloadTables };
constexpr int kResidentEntries = 13;
// the facts of the handle, as plain values: a handle was given at all; loc_window_upload has left a batch; ... under option "resident_slide"; a
// resident solve has run since the upload; the table of full information matrices describes fewer windows than the batch has; the structural
// verdict as it holds now (LOC_WINDOW_KERNEL_*); the three table and lever-arm switches; loc_window_set_message_config has been called
struct ResidentFacts { bool handle = false, resident = false, mirror_valid = false, solved = false, pinfo_short = false; int topology = 0; bool has_off1 = false, has_pinfo = false, pinfo_translation = false, msg_set = false; };
struct Refusal { int code; const char* text; };   // LOC_OK and nullptr: go on; else the LOC_ERR_* and the words of the FIRST refusal
// arg_failed: 0, or k when the k-th of the entry's own argument checks (NULL arrays, kinds_mask, chi2_max, trajectory_length ..., counted in
// the order the entry takes them) is the first of them to fail: the rule knows where each sits between the state checks, and its words
Refusal resident_refusal(ResidentEntry e, const ResidentFacts& f, int arg_failed);

}  // namespace locamd
