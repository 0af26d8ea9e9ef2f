// The dispatch rules of the batched sliding-window solver (window_dispatch.h).  Host code only: no HIP call, no environment, no handle.
#include "window_dispatch.h"
#include "window_layouts.h"

#include "../../include/localization_amd.h"

namespace locamd {

// what only the general kernel evaluates: lever arms on endpoint 1, full information matrices on the priors.  One flag of the structure
// hash and of build_tree_sched: no cached verdict and no forest schedule survives a change of it.
bool general_only(const DispatchOpts& o) { return o.has_off1 || o.has_pinfo; }
// ... unless the table is a dense 3 x 3 block on the translations and the handle asked for the 3 x 3 kernels: wave3_lm_kernel<JAC, true> and
// covariance_kernel<3, .., true> take such a table on a translation-only chain (pick_kernel, structured_covariance_kind); chain3_lm_kernel,
// arrow3_lm_kernel and every other pass do not
bool structured_pinfo(const DispatchOpts& o) { return o.pinfo_structured && o.has_pinfo && o.pinfo_translation && !o.has_off1; }

// Large batches of CHAIN windows (every pose-to-pose edge — range or SE3 — joins consecutive poses; edges ordered by their
// later pose and priors by pose — the order Localization::addRangeEdge / addImuEdge create them in) run one lane per window
// (chain_lm_kernel; chain3_lm_kernel when the batch is translation-only).  Below the threshold a wave per window is faster (the
// lane-per-window kernels take about as long for 1 000 windows as for 65 536); LOCAMD_CHAIN_MIN_BATCH in the environment moves it
// (0 = never), loc_window_set_chain_threshold / option "chain_min_batch" the handle's.
long long effective_chain_min(const DispatchOpts& o) { return o.chain_min >= 0 ? o.chain_min : o.env_chain_min; }

long long tree_min_batch(const DispatchOpts& o) {
    const long long mn = effective_chain_min(o);
    if (mn <= 0) return 1ll << 62;     // (threshold 0 = "never a batch kernel")
    return mn < 256 ? mn : 256;
}

DispatchFits dispatch_fits(const WindowCaps& c) {
    DispatchFits f;
    f.nv_max = c.nv_max;
    f.wave6 = wave6_fits(c, false);
    f.wave6_se3 = wave6_fits(c, true);
    f.wave3 = wave3_fits(c, false);
    f.wave3_pinfo = wave3_fits(c, true);
    f.cov_chain = cov_chain_fits(c, false);
    f.cov_arrow = cov_arrow_fits(c);
    f.cov_envelope = cov_envelope_fits(c);
    return f;
}

// option "arrow3" admits the batch: 0 = never, 1 = whenever it qualifies; default: windows of more than 64 poses — below that the
// wave-per-window kernel keeps everything in LDS and is the better choice
bool arrow3_wanted(const DispatchOpts& o, const DispatchFits& f) { return o.arrow3 >= 0 ? o.arrow3 == 1 : f.nv_max > 64; }

bool forest_groups_wanted(const DispatchOpts& o, const WindowCaps& c, int64_t n) {
    return o.forest_groups && o.tree != 0 && o.tree != 2 && n >= tree_min_batch(o) && c.nv_max <= 64 && !general_only(o);
}

// what the batch qualifies for BY ITS STRUCTURE: LOC_WINDOW_KERNEL_GENERAL, _CHAIN (block-tridiagonal, 6-DoF), _CHAIN3, _WAVE6, _WAVE6S,
// _ARROW3, _TREE or _TREE_GROUPS.  aux: the set of host-built tables that ARROW3 (row order, packed edge records) / TREE (the schedule) fill.
// Host-path calls (tc != nullptr; the resident batch passes none) keep the structural verdict of the previous batch in *tc: the same counts
// and index tables (one 64-bit hash; a collision — 2^-64 per call — would hand a batch to a kernel built for another structure) skip the tests below.
// What depends on the VALUES (translation_only: identity rotations, zero lever arms; arrow3's packed edge records) is looked at every time.
Topology batch_topology(const WindowCaps& c, const DispatchOpts& o, const DispatchFits& f, int n_anchors, const HostBatch& b, WinAux& aux, TopoCache* tc) {
    const bool use_cache = tc && o.topology_cache;
    unsigned long long key = 0;
    bool hit = false;
    if (use_cache) {
        key = hash_structure(c, general_only(o), b);
        hit = tc->valid && tc->key == key && tc->n == b.n;
    }
    bool chain = true;
    bool single_pairs = true;   // no EdgeSE3 anywhere and at most one range edge per pair of consecutive poses (wave6_lm_kernel's rank-1 couplings)
    bool se3_pairs = false;     // EdgeSE3 factors, at most one per pair of consecutive poses, and at most one range edge per pair (wave6_lm_kernel<JAC, true>)
    if (hit) { chain = tc->chain; single_pairs = tc->single_pairs; se3_pairs = tc->se3_pairs; }
    if (!hit) chain_scan(c, b, true, chain, single_pairs, se3_pairs);
    if (use_cache && !hit) { tc->valid = true; tc->key = key; tc->n = b.n; tc->chain = chain; tc->single_pairs = single_pairs; tc->se3_pairs = se3_pairs; tc->tree_tried = false; tc->tree_ok = false; tc->groups_tried = false; tc->groups_ok = false; }
    if (chain) {
        // (under a structured table the priors' diagonals are not read by any kernel, so not by the scan either: the verdict holds while
        //  structured_pinfo does — pick_kernel asks again, and the resident batch remembers how its verdict was taken)
        if (translation_only(c, n_anchors, b, structured_pinfo(o))) return {LOC_WINDOW_KERNEL_CHAIN3, hit};
        if (single_pairs && f.wave6) return {LOC_WINDOW_KERNEL_WAVE6, hit};
        // cfg/uwb_twist.yaml's window: a twist EdgeSE3 per consecutive pair next to the ranges — the wave-per-window kernel with full coupling
        // blocks.  (The same window was tried on tree_wave_kernel first — a chain is a forest, rooted at its centre it has 8 levels: 0.58 … 0.67 ms
        // per solve against the general kernel's 0.62 ms, tools/dev/probe_tree_chain.py: no speculative trials, one or two busy lanes per level.)
        if (se3_pairs && f.wave6_se3) return {LOC_WINDOW_KERNEL_WAVE6S, hit};   // (nv + 1 lanes: the middle pose twice)
        return {LOC_WINDOW_KERNEL_CHAIN, hit};
    }
    if (arrow3_wanted(o, f) && translation_only(c, n_anchors, b) && build_arrow_aux(c, b, aux)) return {LOC_WINDOW_KERNEL_ARROW3, hit};
    // (option "tree" = 0: never.  One wave per window, so any batch gains; the host-side comparison of the index tables is only worth
    //  it from a few hundred windows on — or from the chain threshold when that was lowered, as the tests do)
    if (o.tree != 0 && b.n >= tree_min_batch(o)) {
        if (hit && tc->tree_tried) {
            if (tc->tree_ok) return {LOC_WINDOW_KERNEL_TREE, hit};   // (aux's schedule is still the one built for this structure)
        } else {
            const bool ok = build_tree_sched(c, general_only(o), b, aux);
            if (use_cache) { tc->tree_tried = true; tc->tree_ok = ok; }
            if (ok) return {LOC_WINDOW_KERNEL_TREE, hit};
        }
        // option "forest_groups": forest windows of differing topologies, only after build_tree_sched has declined the batch — a one-topology batch
        // takes the path above.  Never under option "tree" = 2 (tree_lm_kernel has no per-window-schedule twin) or on a handle of longer windows.
        // On a hit aux's groups and tables are still those built for this structure (hash_structure covers the full index tables).
        if (forest_groups_wanted(o, c, b.n)) {   // (under general_only build_tree_groups refuses the batch itself, as build_tree_sched above)
            if (hit && tc->groups_tried) {
                if (tc->groups_ok) return {LOC_WINDOW_KERNEL_TREE_GROUPS, hit};
            } else {
                const bool ok = build_tree_groups(c, general_only(o), b, aux);
                if (use_cache) { tc->groups_tried = true; tc->groups_ok = ok; }
                if (ok) return {LOC_WINDOW_KERNEL_TREE_GROUPS, hit};
            }
        }
    }
    return {LOC_WINDOW_KERNEL_GENERAL, hit};
}

// batch_topology's chain block on the flags of a batch no host pass has seen (window_dispatch.h); nothing else is decided here
int topology_from_flags(const DispatchOpts& o, const DispatchFits& f, const WindowBatchFlags& b) {
    if (!b.chain) return LOC_WINDOW_KERNEL_GENERAL;
    if (structured_pinfo(o) ? b.translation_only_skip : b.translation_only) return LOC_WINDOW_KERNEL_CHAIN3;
    if (b.single_pairs && f.wave6) return LOC_WINDOW_KERNEL_WAVE6;
    if (b.se3_pairs && f.wave6_se3) return LOC_WINDOW_KERNEL_WAVE6S;
    return LOC_WINDOW_KERNEL_CHAIN;
}

static int pick_plain(const DispatchOpts& o, const DispatchFits& f, int64_t n, int topology);

int pick_kernel(const DispatchOpts& o, const DispatchFits& f, int64_t n, int topology) {
    if (general_only(o)) {   // (lever arms on endpoint 1, full-information priors: only the general kernel evaluates them ...
        // ... but for a structured table on a translation-only chain that the handle's other switches would hand to wave3_lm_kernel: its twin
        // <JAC, true> takes it, when its larger prior records fit)
        if (structured_pinfo(o) && topology == LOC_WINDOW_KERNEL_CHAIN3 && f.wave3_pinfo) {
            DispatchFits g = f;
            g.wave3 = true;
            if (pick_plain(o, g, n, topology) == LOC_WINDOW_KERNEL_WAVE3) return LOC_WINDOW_KERNEL_WAVE3;
        }
        return LOC_WINDOW_KERNEL_GENERAL;
    }
    return pick_plain(o, f, n, topology);
}

// the rule for handles without lever arms on endpoint 1 and without a table of full information matrices
static int pick_plain(const DispatchOpts& o, const DispatchFits& f, int64_t n, int topology) {
    const long long mn = effective_chain_min(o);
    const bool default_rule = o.chain_min < 0 && !o.env_chain_min_set;
    if (mn <= 0 || o.natural_order) return LOC_WINDOW_KERNEL_GENERAL;   // threshold 0 = "never anything but the general kernel" (every structure)
    if (topology == LOC_WINDOW_KERNEL_WAVE6 || topology == LOC_WINDOW_KERNEL_WAVE6S) {   // (WAVE6S: the same rule for chains with EdgeSE3 factors)
        // a 6-DoF chain batch that also qualifies for wave6_lm_kernel (one wave per window, rank-1 couplings).  Measured on twelve-pose
        // cfg/uwb_imu.yaml windows: 1.15e7 windows/s at 4 096, 16 384 and 65 536 windows against chain_lm_kernel's 1.1e6 / 4.3e6 / 6.9e6 —
        // so by default it takes every batch; an explicit threshold hands batches from that size on to the lane-per-window kernel.
        // option "wave6" = 0: as before (the general kernel below the threshold, chain_lm_kernel from it on), for A/B runs.
        const bool off = !o.wave6;
        if (n >= mn && (off || !default_rule)) return LOC_WINDOW_KERNEL_CHAIN;
        return off ? LOC_WINDOW_KERNEL_GENERAL : topology;
    }
    if (topology == LOC_WINDOW_KERNEL_ARROW3) return LOC_WINDOW_KERNEL_ARROW3;   // (one workgroup per window: any batch size)
    if (topology == LOC_WINDOW_KERNEL_TREE) return n < tree_min_batch(o) ? LOC_WINDOW_KERNEL_GENERAL : LOC_WINDOW_KERNEL_TREE;
    // (the grouped forest: TREE's threshold; a verdict taken under switches that have changed since — a resident batch's — falls to the general kernel)
    if (topology == LOC_WINDOW_KERNEL_TREE_GROUPS) return n < tree_min_batch(o) || !o.forest_groups || o.tree == 0 || o.tree == 2 ? LOC_WINDOW_KERNEL_GENERAL : LOC_WINDOW_KERNEL_TREE_GROUPS;
    if (topology == LOC_WINDOW_KERNEL_CHAIN3 && f.wave3) {
        // translation-only chains of <= 64 poses (the node's single window first of all): one wave per window with 3x3 blocks, rank-1
        // couplings and speculative LM trials.  Measured on ten-pose windows: 0.056 ms for one window, 3.6e7 windows/s (numeric) /
        // 4.0e7 (analytic) from ~8 000 windows on — level with chain3_lm_kernel at 65 536 windows, ahead of it everywhere else — so by
        // default it takes every batch; an explicit threshold (loc_window_set_chain_threshold / LOCAMD_CHAIN_MIN_BATCH) hands batches
        // from that size on to the lane-per-window kernel.  Options "wave3" / "chain3" = 0: no such kernel (A/B runs, tests).
        if ((default_rule || n < mn) && o.wave3 && o.chain3) return LOC_WINDOW_KERNEL_WAVE3;
    }
    if (topology == LOC_WINDOW_KERNEL_CHAIN3 && default_rule && n >= 4096 && n < mn) {
        // the translation-only kernel is worth it from ~4 096 windows on (it takes ~1 ms for any batch up to 16 384, the wave-per-window
        // kernel 4.3e6 windows/s): e.g. one GPU's 8 192-window share of a 65 536-window job split over eight
        if (o.chain3) return LOC_WINDOW_KERNEL_CHAIN3;
    }
    if (topology == LOC_WINDOW_KERNEL_GENERAL || n < mn) return LOC_WINDOW_KERNEL_GENERAL;
    if (topology == LOC_WINDOW_KERNEL_CHAIN3 && !o.chain3) return LOC_WINDOW_KERNEL_CHAIN;   // the 6-DoF kernel on a translation-only batch (A/B runs, tests)
    return topology;
}

// The pass a batch's covariances are computed by, structured passes only; CovKind::None = not covered: lever arms on endpoint 1, or a batch
// none of the three tests below takes.  In this order:
// 1. windows of <= 64 poses that are chains (in any edge order): Chain3 for translation-only batches, Chain6 otherwise (covariance_kernel.hip);
// 2. Arrow when the handle would solve the batch on arrow3_lm_kernel (batch_topology's rule: arrow3_wanted — by default windows of
//    more than 64 poses only —, translation_only, build_arrow_aux's verdict) — arrow_covariance_kernel.hip; the structure test runs on `own`,
//    a table set of the covariance's own, and the list size goes to the verdict's list_cap;
// 3. windows of <= 64 poses: ForestOwn when the handle would solve the batch on a forest kernel (batch_topology's rule: option "tree",
//    tree_min_batch, build_tree_sched's verdict) — forest_covariance_kernel.hip on the schedule built into `own`, which the caller then sends
//    to the device (need_upload).  keyed (the host path): the set is kept with the hash of the structure it was built for, and a batch of
//    the same structure reuses it, device copy included.
// 3b. only after build_tree_sched has declined: ForestGroupsOwn when options "forest_groups" and "forest_groups_covariance" are both 1 and the
//    handle would solve the batch on the grouped kernel (forest_groups_wanted, build_tree_groups' verdict: no window with nv < 2, no cycle, at
//    most one EdgeSE3 per pair) — forest_covariance_groups_kernel.hip on the groups block built into `own` (need_upload).  keyed: the key
//    remembers WHICH of the two table sets it holds; a hit returns that kind, and a grouped one only while the two options still hold.
static CovVerdict structured_covariance_kind(const WindowCaps& c, const DispatchOpts& o, const DispatchFits& f, int n_anchors, const HostBatch& b,
                                             WinAux& own, SchedKey* keyed) {
    const CovVerdict none{CovKind::None, false, 0, 0};
    // (full-information priors: the three passes below read the diagonals alone — the envelope pass serves them; a structured table on a
    //  translation-only chain alone is the chain pass's, covariance_kernel<3, .., true>)
    const bool structured = structured_pinfo(o);
    if (general_only(o) && !structured) return none;
    const bool small = c.nv_max <= 64;
    if (small) {
        bool chain = false, single_pairs = false, se3_pairs = false;
        chain_scan(c, b, false, chain, single_pairs, se3_pairs);
        if (chain) {
            if (!f.cov_chain) return none;
            if (structured) return {translation_only(c, n_anchors, b, true) ? CovKind::Chain3 : CovKind::None, false, 0, 0};
            return {translation_only(c, n_anchors, b) ? CovKind::Chain3 : CovKind::Chain6, false, 0, 0};
        }
    }
    if (structured) return none;
    if (arrow3_wanted(o, f) && f.cov_arrow && translation_only(c, n_anchors, b) && build_arrow_aux(c, b, own, true))
        return {CovKind::Arrow, false, own.arrow_list_cap, 0};
    if (!small) return none;
    if (o.tree == 0 || b.n < tree_min_batch(o)) return none;
    const bool groups = o.forest_groups_cov && forest_groups_wanted(o, c, b.n);
    if (keyed) {
        const unsigned long long key = hash_structure(c, general_only(o), b);
        if (keyed->valid && keyed->key == key && keyed->n == b.n) {
            if (keyed->kind == CovKind::ForestOwn) return {CovKind::ForestOwn, false, 0, 0};
            // (a groups block: build_tree_sched declined this structure when it was built, and does so again)
            if (keyed->kind == CovKind::ForestGroupsOwn) return groups ? CovVerdict{CovKind::ForestGroupsOwn, false, 0, 0} : none;
        }
        keyed->valid = false;   // (valid again once the caller has uploaded the new tables)
        keyed->key = key; keyed->n = b.n; keyed->kind = CovKind::None;
    }
    if (build_tree_sched(c, general_only(o), b, own)) {
        if (keyed) keyed->kind = CovKind::ForestOwn;
        return {CovKind::ForestOwn, true, 0, 0};
    }
    if (!groups || !build_tree_groups(c, general_only(o), b, own)) return none;
    if (keyed) keyed->kind = CovKind::ForestGroupsOwn;
    return {CovKind::ForestGroupsOwn, true, 0, 0};
}

long long cov_switches(const DispatchOpts& o) {
    const long long mn = tree_min_batch(o);
    return (((long long)(o.arrow3 + 1) << 4 | (long long)(o.tree + 1)) ^ ((mn > (1ll << 40) ? (1ll << 40) : mn) << 8)) | (o.has_pinfo ? 1ll << 60 : 0) |
           (o.pinfo_structured ? 1ll << 59 : 0) | (o.has_pinfo && o.pinfo_translation ? 1ll << 58 : 0) | (o.forest_groups && o.forest_groups_cov ? 1ll << 57 : 0);
}

// 4. option "covariance_general" = 1: whatever the tests above leave (no endpoint-1 lever arms) is Envelope —
//    envelope_covariance_kernel.hip in the caller's pose order; the batch's largest envelope goes to the verdict's env_blocks.
//    pt: the pairs of a joint call count as edges of that envelope (none: the plain envelope).
CovVerdict covariance_kind(const WindowCaps& c, const DispatchOpts& o, const DispatchFits& f, int n_anchors, const HostBatch& b, const PairTables& pt,
                           WinAux& own, SchedKey* keyed) {
    const CovVerdict v = structured_covariance_kind(c, o, f, n_anchors, b, own, keyed);
    if (v.kind != CovKind::None || o.has_off1 || !o.cov_general) return v;
    if (!f.cov_envelope) return v;
    const long long blocks = envelope_blocks_max_joint(c, b, pt);
    if (blocks < 0) return v;   // (cannot happen: the tables were validated)
    return {CovKind::Envelope, false, 0, blocks};
}

// (a forest batch is served while the handle would solve it on a forest kernel: the threshold is looked at per call, as pick_kernel does)
// (an arrowhead batch likewise while option "arrow3" still admits it; the envelope pass while option "covariance_general" is 1)
bool cov_admitted(const DispatchOpts& o, const DispatchFits& f, int64_t n, CovKind kind) {
    const bool groups = kind == CovKind::ForestGroups || kind == CovKind::ForestGroupsOwn;
    const bool forest = kind == CovKind::Forest || kind == CovKind::ForestOwn || groups;
    const bool arrow = kind == CovKind::Arrow, envelope = kind == CovKind::Envelope;
    const bool refused = o.has_off1 || (o.has_pinfo && !envelope && !(kind == CovKind::Chain3 && structured_pinfo(o))) || (f.nv_max > 64 && !arrow && !envelope) || kind == CovKind::Unclassified || kind == CovKind::None ||
                         (forest && (n < tree_min_batch(o) || o.tree == 0)) || (arrow && (!arrow3_wanted(o, f) || !f.cov_arrow)) || (envelope && !o.cov_general) ||
                         (groups && (!o.forest_groups || !o.forest_groups_cov || o.tree == 2));   // (the grouped forest: both options, and the solve's own rule)
    return !refused;
}

int cov_public_kind(CovKind kind) {
    switch (kind) {
        case CovKind::Chain3: return LOC_WINDOW_COV_CHAIN3;
        case CovKind::Chain6: return LOC_WINDOW_COV_CHAIN6;
        case CovKind::Forest: case CovKind::ForestOwn: return LOC_WINDOW_COV_FOREST;
        case CovKind::Arrow: return LOC_WINDOW_COV_ARROW;
        case CovKind::Envelope: return LOC_WINDOW_COV_ENVELOPE;
        case CovKind::ForestGroups: case CovKind::ForestGroupsOwn: return LOC_WINDOW_COV_FOREST_GROUPS;
        default: return LOC_WINDOW_COV_NONE;
    }
}

CovKind resident_groups_covariance(const DispatchOpts& o, const DispatchFits& f, int64_t n, bool groups_no_chain) {
    return groups_no_chain && cov_admitted(o, f, n, CovKind::ForestGroups) ? CovKind::ForestGroups : CovKind::Unclassified;
}

bool cov_stale(const DispatchOpts& o, const DispatchFits& f, int64_t n, CovKind kind, long long env_switches) {
    // (the envelope pass holds the batch only while the three structured tests would still decline it — they are run again when a
    //  switch they read has changed, so that the resident batch takes the pass loc_window_covariance_host takes)
    if (kind == CovKind::Envelope) return env_switches != cov_switches(o);
    // (option "covariance_general": a structured verdict the handle's switches no longer admit is no verdict — the batch is classified under
    //  the switches as they are now, and lands on the envelope pass)
    return kind != CovKind::Unclassified && kind != CovKind::None && o.cov_general && !o.has_off1 && !cov_admitted(o, f, n, kind);
}

// ---- the resident entries' refusals ("What every resident entry refuses") --------------------------------------------------------
#define LOC_UNSOLVED(who) who ": no resident solve has run since the upload"
#define LOC_SLIDE_ROWS "loc_window_slide_resident: new pose and new row arrays"
#define LOC_MESSAGE_ARGS "loc_window_message_rows: kinds_mask has unknown bits", "loc_window_message_rows: kind and dt arrays", "loc_window_message_rows: a NULL message array under a bit of kinds_mask"
enum RefusalText { kNothing, kNothingPublish, kNothingPath, kMirror, kMsgSet, kPinfoShort, kSlideVerdict, kSlideOff1, kSlidePinfoRotation, kPlainChain3, kPlainVerdict, kPlainPinfo, kPruneArrow3,
                   kUnsolved /* + entry */, kRefusalTexts = kUnsolved + kResidentEntries };
static const char* const kRefusalText[kRefusalTexts] = {
    "nothing uploaded", "loc_window_publish_resident: nothing uploaded", "loc_window_path_resident: nothing uploaded",
    "loc_window_slide_resident: option \"resident_slide\" was 0 when the batch was uploaded", "loc_window_message_rows: loc_window_set_message_config has not been called",
    "the resident batch has more windows than loc_window_set_prior_information described",
    "loc_window_slide_resident: the resident batch is not an ordered translation-only chain batch", "loc_window_slide_resident: no endpoint-1 lever arms",
    "loc_window_slide_resident: the table of full information matrices has rotation entries",
    "loc_window_slide_plain_resident_dev: the resident batch is an ordered translation-only chain batch: loc_window_slide_resident / loc_window_slide_resident_dev slide it",
    "loc_window_slide_plain_resident_dev: the resident batch is not an ordered 6-DoF chain batch", "loc_window_slide_plain_resident_dev: the handle has a table of full information matrices",
    "loc_window_prune_resident: the resident batch is solved by arrow3_lm_kernel from records packed at upload",
    nullptr, LOC_UNSOLVED("loc_window_download"), LOC_UNSOLVED("loc_window_covariance_resident"), LOC_UNSOLVED("loc_window_slide_resident"), LOC_UNSOLVED("loc_window_slide_resident"),
    LOC_UNSOLVED("loc_window_slide_resident"), LOC_UNSOLVED("loc_window_message_rows"), LOC_UNSOLVED("loc_window_message_rows"), LOC_UNSOLVED("loc_window_edge_chi2_resident"),
    LOC_UNSOLVED("loc_window_prune_resident"), LOC_UNSOLVED("loc_window_publish_resident"), LOC_UNSOLVED("loc_window_path_resident"), nullptr};
// the words of the entries' own argument checks (the checks stay with the entries), in the order each entry takes them
static const char* const kArgumentText[kResidentEntries][4] = {
    {}, {}, {"covariance output arrays"}, {LOC_SLIDE_ROWS}, {LOC_SLIDE_ROWS}, {LOC_SLIDE_ROWS},
    {LOC_MESSAGE_ARGS, "loc_window_message_rows_dev: a NULL output array (only verdict may be NULL)"}, {LOC_MESSAGE_ARGS}, {},
    {"loc_window_prune_resident: chi2_max must be a number >= 0 and min_edges >= 0"},
    {"loc_window_publish_resident: minimum_optimize_error is NaN", "loc_window_publish_resident: flags_dev is NULL", "loc_window_publish_resident: trajectory_length must be in [1, nv_max]"},
    {"loc_window_path_resident: path_dev or present_dev is NULL", "loc_window_path_resident: first >= 0, count >= 1 and first + count <= trajectory_length are required",
     "loc_window_path_resident: trajectory_length must be in [1, nv_max]"},
    {"loc_window_download_tables: the handle has no table of full information matrices"}};

// The order, for every entry: [publish, path: their first two argument checks] — handle and batch — [the slides: the mirror] [the message
// entries: the configuration] — solved (but the solve and the tables' download) — the argument checks that are left (prune's comes later) —
// [push: the mirror] — the table covers the batch (but the downloads, the build, publish and path) — [prune: its argument check, then the
// verdict] — [the slides and push: the verdict, the lever arms, the table, as the carrying or the plain slide wants them]
Refusal resident_refusal(ResidentEntry e, const ResidentFacts& f, int arg_failed) {
    using E = ResidentEntry;
    auto no = [](int code, int text) { return Refusal{code, kRefusalText[text]}; };
    const Refusal go{LOC_OK, nullptr}, argument{LOC_ERR_INVALID, arg_failed >= 1 && arg_failed <= 4 ? kArgumentText[(int)e][arg_failed - 1] : nullptr};
    if (!argument.text) arg_failed = 0;   // (the entry has no such check)
    const bool records = e == E::Publish || e == E::Path, slide = e == E::SlideHost || e == E::SlideDev || e == E::SlidePlain;
    if (records && (arg_failed == 1 || arg_failed == 2)) return argument;
    if (!f.handle || !f.resident) return no(LOC_ERR_INVALID, e == E::Publish ? kNothingPublish : e == E::Path ? kNothingPath : kNothing);
    if (slide && !f.mirror_valid) return no(LOC_ERR_INVALID, kMirror);
    if ((e == E::MessageRows || e == E::PushMessages) && !f.msg_set) return no(LOC_ERR_INVALID, kMsgSet);
    if (e != E::Solve && e != E::DownloadTables && !f.solved) return no(LOC_ERR_INVALID, kUnsolved + (int)e);
    if (arg_failed && e != E::Prune) return argument;
    if (e == E::PushMessages && !f.mirror_valid) return no(LOC_ERR_INVALID, kMirror);
    if (e == E::Download || e == E::DownloadTables || e == E::MessageRows || records) return go;
    if (f.pinfo_short) return no(LOC_ERR_INVALID, kPinfoShort);
    if (e == E::Prune) {
        if (arg_failed) return argument;
        // build_arrow_aux packed measurement and information into ArrowAux::rec at upload: a store into r_val would not reach that solve
        // (every other solve kernel and covariance pass reads range values from r_val at launch)
        return f.topology == LOC_WINDOW_KERNEL_ARROW3 ? no(LOC_ERR_UNSUPPORTED, kPruneArrow3) : go;
    }
    if (!slide && e != E::PushMessages) return go;
    const int t = f.topology;
    if (e == E::SlidePlain || (e == E::PushMessages && t != LOC_WINDOW_KERNEL_CHAIN3)) {
        // the plain drop: one of the ordered 6-DoF chain verdicts, and no table of full information matrices at all
        if (t == LOC_WINDOW_KERNEL_CHAIN3) return no(LOC_ERR_UNSUPPORTED, kPlainChain3);
        if (t != LOC_WINDOW_KERNEL_CHAIN && t != LOC_WINDOW_KERNEL_WAVE6 && t != LOC_WINDOW_KERNEL_WAVE6S) return no(LOC_ERR_UNSUPPORTED, kPlainVerdict);
        if (f.has_off1) return no(LOC_ERR_UNSUPPORTED, kSlideOff1);
        return f.has_pinfo ? no(LOC_ERR_UNSUPPORTED, kPlainPinfo) : go;
    }
    if (t != LOC_WINDOW_KERNEL_CHAIN3) return no(LOC_ERR_UNSUPPORTED, kSlideVerdict);
    if (f.has_off1) return no(LOC_ERR_UNSUPPORTED, kSlideOff1);
    return f.has_pinfo && !f.pinfo_translation ? no(LOC_ERR_UNSUPPORTED, kSlidePinfoRotation) : go;
}

}  // namespace locamd
