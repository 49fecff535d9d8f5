// Internal launch interface between hgi_qviews.hip (entry point, argument checks) and hgi_fused_qviews.hip (kernels).
#pragma once
#include "../csrc/hgi_kernels.h"
#include "hgi_qviews_plan.h"

namespace hgi {

// One launch: the tiles of every grid of the list, k fused levels (1 ... kFusedMaxLevels) in both directions and, with up >= 1
// (k == 4 only), the cone that rebuilds the `up` <= 4 levels above a tile from the source grid through its read pitch.
// a: the arrays of the DEVICE blob of a view list's plan; a.count >= 1 and the block count fits (views_info_consistent).  The
// table is not the identity.
hipError_t launch_qviews_requant(const ViewArgs &a, uint32_t k, uint32_t up, int interp, const Lut256 &lut, hipStream_t s);

}  // namespace hgi
