// gfx950 (MI355X / CDNA4): forest_covariance_kernel<JAC, JOINT, TreeGroups> — marginal pose covariances and cross blocks of forest windows of
// DIFFERING topologies (option "forest_groups_covariance"), one wave per window on the schedule of the window's group.  The kernel is
// forest_covariance_kernel.hip's, word for word: this unit instantiates it for the second schedule type and holds its launcher
// (launch_window_forest_covariance_groups).  A unit of its own so that the TreeSched instantiations stay alone in their module.
#define LOCAMD_FOREST_COV_GROUPS 1
#include "forest_covariance_kernel.hip"
