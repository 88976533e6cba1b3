// hq_cost_masked.hip -- hq_cost.hip's kernels once more as their masked
// instances (MSK: the pixel mask of hq_set_mask in the reduction, the work items
// through the live-tile list) and the launchers that name them,
// launch_cost_fast_masked and launch_cost_chunked_masked.  A translation unit
// of its own, so the plain instances' source and build stay what they were.
#define HQ_COST_MASKED 1
#include "hq_cost.hip"
