// hq_cost_weighted.hip -- hq_cost.hip's kernels once more as their weighted
// instances (MSK = 2: the pixel weights of hq_set_weights in the reduction, one
// fma per pixel; the work items through the live-tile list) and the launchers
// that name them, launch_cost_fast_weighted and launch_cost_chunked_weighted.  A
// translation unit of its own, like hq_cost_masked.hip, so the plain and masked
// instances' source and build stay what they were.
#define HQ_COST_WEIGHTED 1
#include "hq_cost.hip"
