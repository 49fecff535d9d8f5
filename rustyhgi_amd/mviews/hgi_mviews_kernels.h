// Internal launch interface between hgi_mviews.hip (entry points, argument checks, plan) and hgi_fused_mviews_dec.hip (kernels).
#pragma once
#include "../csrc/hgi_kernels.h"
#include "hgi_mviews_plan.h"

namespace hgi {

// One launch: the tiles of every frame of the list, k fused levels (1 ... kFusedMaxLevels) and, with up >= 1 (k == 4 only), the
// cone that rebuilds the `up` <= 4 levels above a tile from the grid's own samples through its read pitch.  a: the arrays of the
// DEVICE blob; a.count >= 1 and the block count fits (mviews_info_consistent).  max_width: the widest frame (the decoder's
// occupancy policy).  `table`: 256 elements of `elem` (2 or 4) bytes in device memory.
hipError_t launch_mviews_decode(const ViewArgs &a, uint32_t max_width, const void *table, uint32_t elem, uint32_t k, uint32_t up, int interp,
                                hipStream_t s);

}  // namespace hgi
