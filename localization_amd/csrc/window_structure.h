// Structure analysis of a batch of windows, free of any handle state (each pass is described at its definition in window_structure.cpp)
#pragma once
#include <vector>

#include "window_kernel.h"
#include "window_tables.h"

namespace locamd {

// Host-built tables (tree_wave / tree_lm: the elimination schedule; arrow3: row order + packed edge records): build_tree_sched /
// build_arrow_aux fill the host vectors and the sizes, capi_window.cpp owns the device copies.
struct WinAux {
    int32_t* d_tsched = nullptr;
    size_t tsched_cap = 0;
    std::vector<int32_t> h_tsched;
    TreeSched tsched{};
    // option "forest_groups" (build_tree_groups): the block [hdr | sched_of | pad | tables] of window_kernel.h's TreeGroups, its device copy,
    // the number of groups (0: the batch is not on the grouped path) and where sched_of and the tables start (int32s)
    std::vector<int32_t> h_groups;
    int32_t* d_groups = nullptr;
    size_t groups_cap = 0, groups_of_at = 0, groups_tab_at = 0;
    int n_groups = 0;
    int32_t *d_ahdr = nullptr, *d_arslot = nullptr;
    double *d_arec = nullptr, *d_aprec = nullptr;
    size_t arec_cap = 0, aprec_cap = 0;   // doubles allocated
    int arrow_nb_max = 0, arrow_jmax = 0, arrow_jpmax = 0, arrow_list_cap = 0;
    int arrow_jch[16] = {0}, arrow_jpch[16] = {0};   // records per chunk of 64 rows (the most any row of the chunk has, over the batch)
    std::vector<int32_t> h_ahdr, h_arslot;
    std::vector<double> h_arec, h_aprec;
};

// 0, or the first check that failed: 1 counts exceed the capacities, 2 / 3 range edge (vertex index / poses further apart than bw_max),
// 4 prior edge vertex index, 5 / 6 SE3 edge (as 2 / 3)
int check_instances(const WindowCaps& c, int n_anchors, const HostBatch& b);
// the largest anchor the range rows of n checked instances reference, as -v1 (v1 = -1 - anchor; 0: none): counts [n][4], r_idx [n][nr_max][2],
// rows beyond an instance's count are not read
int max_anchor_referenced(const WindowCaps& c, int64_t n, const int32_t* counts, const int32_t* r_idx);
// skip_prior_diagonal: the priors' information comes from a full-matrix table (loc_window_set_prior_information), p_val's diagonal is not read
bool translation_only(const WindowCaps& c, int n_anchors, const HostBatch& b, bool skip_prior_diagonal = false);
// the full information matrices of n_rows priors ([n_rows][36]) carry no rotation information: rows and columns 3 .. 5 exactly 0
bool prior_information_translation_only(size_t n_rows, const double* pinfo);
// the drop slots of a marginal-prior call (loc_window_marginal_prior_host), drop [n]; the batch's tables are already checked
// (check_instances).  0, or the first check that failed: 1 a drop slot outside [0, nv) of its window; 2 pose-to-pose ranges join some
// window's dropped pose to more than one other pose (a marginal over several poses is not a unary prior: arrowheads are such windows) —
// several ranges to the same pose, in either direction, are one neighbour
int check_marginal_drop(const WindowCaps& c, const HostBatch& b, const int32_t* drop);
// The integer half of the resident slide (loc_window_slide_resident; DESIGN.md §2, "The resident slide") on the host's mirror of an ordered
// translation-only chain batch: counts [n][4], r_idx [n][nr_max][2], p_idx [n][np_max].  Per window: drop[b] != 0 (drop == nullptr: every
// window) removes slot 0, the range rows with it as an endpoint and the prior rows on it, renumbers the moving slots, and puts the carried
// prior (row 0 on slot 0) in front of the kept priors iff a pose-to-pose range joined slot 0 to another pose; then the new slot s, r_counts[b]
// rows of r_idx [n][nr_new_max][2] and p_counts[b] prior rows on s are appended.
// apply == false: nothing is written.  bad = 0, or the first check that failed: 1 a window with nv = 0; 2 a new count outside [0, *_new_max];
// 3 a new range index outside the rule (v0 in {s - 1, s}; v1 in {s - 1, s} or an anchor code of [0, n_anchors); v0 != v1; a pose-to-pose row
// needs bw_max >= 1; no row on s - 1 alone after a row that names s); 4 / 5 / 6 the slid window exceeds nv_max / nr_max / np_max.
// apply == true (after a call that returned bad = 0 for the same arguments): the mirror is rewritten in place; max_anchor = the largest
// anchor code referenced afterwards, as -v1 (0: none).
struct SlideRows { const int32_t* drop; int32_t nr_new_max; const int32_t* r_counts; const int32_t* r_idx; int32_t np_new_max; const int32_t* p_counts; };
struct SlideVerdict { int bad; int max_anchor; };
SlideVerdict slide_indices(const WindowCaps& c, int n_anchors, int64_t n, int32_t* counts, int32_t* r_idx, int32_t* p_idx, const SlideRows& s, bool apply);
// the value half of that admission: every new row is translation-only — new_pose [n][12] with an identity rotation, r_val [n][nr_new_max][5]
// without lever arm, p_val [n][np_new_max][18] with an identity measurement rotation and no rotation information.  Counts outside their
// range read no row (slide_indices reports them).
bool slide_rows_translation_only(int64_t n, const SlideRows& s, const double* new_pose, const double* r_val, const double* p_val);
void chain_scan(const WindowCaps& c, const HostBatch& b, bool ordered, bool& chain, bool& single_pairs, bool& se3_pairs);
unsigned long long hash_structure(const WindowCaps& c, bool has_off1, const HostBatch& b);
// the largest number of envelope blocks any instance has (envelope_covariance_kernel.hip's profile: sum over the pose slots i of
// i - first[i] + 1, first[i] = the smallest slot a pose-to-pose edge joins to i); reads counts, r_idx and s_idx alone; -1: an index out of range
long long envelope_blocks_max(const WindowCaps& c, const HostBatch& b);
// the pose pairs of a joint covariance call (loc_window_joint_covariance_*), host arrays: counts [n], pairs [n][npair_max][2] pose slots
struct PairTables { int32_t npair_max; const int32_t* counts; const int32_t* pairs; };
// 0, or the first check that failed: 1 a pair count outside [0, npair_max], 2 a pose slot outside [0, nv) of its window.  counts: the
// batch's [n][4] table, already checked (check_instances)
int check_pairs(int64_t n, const int32_t* counts, const PairTables& pt);
// envelope_blocks_max with every requested pair taken as one more pose-to-pose edge (the envelope pass keeps Sigma_ij in the block it adds)
long long envelope_blocks_max_joint(const WindowCaps& c, const HostBatch& b, const PairTables& pt);
bool build_arrow_aux(const WindowCaps& c, const HostBatch& b, WinAux& A, bool structure_only = false);   // fills A.h_a* and A.arrow_*
bool build_tree_sched(const WindowCaps& c, bool has_off1, const HostBatch& b, WinAux& A);                // fills A.h_tsched and A.tsched's sizes
size_t bind_tree_sched(TreeSched& ts, const int32_t* base);   // ts's pointers into a copy of that table at base; returns the table's length
// Forest windows of DIFFERING topologies: groups by topology key (counts, index rows without anchor numbers and robust flags), one
// build_tree_sched table per group; fills A.h_groups, A.n_groups, A.groups_*_at.  false: the batch stays with the general kernel
bool build_tree_groups(const WindowCaps& c, bool has_off1, const HostBatch& b, WinAux& A);
// ... in two parts (build_tree_groups is (a) followed by (b)).  (a) the grouping (window_groups.h states the key): of [n] = every window's
// group, ids in order of first appearance; rep = every group's first window.  false: a window with nv outside [2, 64]
bool group_windows(const WindowCaps& c, const HostBatch& b, std::vector<int32_t>& of, std::vector<int64_t>& rep);
// (b) representatives -> block, for a batch grouped elsewhere (loc_window_upload_dev: window_groups_kernel.hip): reps = the compact batch of
// the G = reps.n representatives in group order (counts and used index rows at the capacities c; no value table is read), of [n] = every
// window's group.  Fills A as build_tree_groups does for the batch the representatives were taken from, refusals included
bool build_tree_groups_block(const WindowCaps& c, bool has_off1, const HostBatch& reps, int64_t n, const int32_t* of, WinAux& A);

}  // namespace locamd
