// The schedule of a wave's window, for the kernels that run one wave per forest window on a host-built elimination schedule
// (tree_wave_kernel.hip: the solve; forest_covariance_kernel.hip: the covariances).  Device code; both kernels take the schedule's type as a
// template parameter and differ between the two types in this one function.
//
// SCHED = TreeSched: the one schedule of the batch, whose r_idx / s_idx sections are every window's rows.
// SCHED = TreeGroups (options "forest_groups" / "forest_groups_covariance"): windows of differing topologies, cut from different robots or at
// different phases of the key cadence of Localization::addPoseEdge (localization.cpp:254-290) — the wave reads its window's group and that
// group's header (wave-uniform loads through blockIdx.x), binds the schedule's pointers from the group's table with the host's own function
// (tree_sched_bind), and points r_idx / s_idx at the window's OWN rows: a group's windows share parents, heights and edge lists, not anchor
// numbers or robust flags, and every index look-up of the kernels — the prologue's, the generic loops', the anchor number, the robust flag —
// goes through these two pointers.  The schedule's sizes are then per-wave values.
#pragma once
#include "window_kernel.h"
#include "window_layouts.h"

namespace locamd {

__device__ __forceinline__ const TreeSched& wave_sched(const TreeSched& ts, const WindowArgs&, long long) { return ts; }
__device__ __forceinline__ TreeSched wave_sched(const TreeGroups& g, const WindowArgs& a, long long inst) {
    const int32_t* h = g.hdr + (size_t)g.sched_of[inst] * kTreeGroupHdr;
    TreeSched ts;
    tree_group_sizes(ts, h);
    tree_sched_bind(ts, g.tables + h[10]);
    ts.r_idx = a.r_idx + (size_t)inst * a.caps.nr_max * 2;
    ts.s_idx = a.s_idx + (size_t)inst * a.caps.ns_max * 4;
    return ts;
}

}  // namespace locamd
