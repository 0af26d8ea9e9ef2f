// gfx950 (MI355X / CDNA4): tree_wave_kernel<JAC, TreeGroups> — forest windows of DIFFERING topologies (option "forest_groups"), one wave per
// window on the schedule of the window's group.  The kernel is tree_wave_kernel.hip's, word for word: this unit instantiates it for the
// second schedule type and holds its launcher (launch_window_tree_wave_groups).  A unit of its own because the TreeSched instantiations
// keep their machine code only while they are alone in their module.
#define LOCAMD_TREE_WAVE_GROUPS 1
#include "tree_wave_kernel.hip"
