// Internal launch interface between hgi_rviews.hip (entry points, argument checks, plan) and hgi_fused_rviews_enc.hip (kernels).
#pragma once
#include "../csrc/hgi_kernels.h"
#include "hgi_rviews_plan.h"

namespace hgi {

// One launch: the tiles of every frame of the list, k fused levels (1 ... kFusedMaxLevels) and, with up >= 1 (k == 4 only), the
// cone that rebuilds the `up` <= 4 levels above a tile from the frame's own samples through its read pitch.  a: the arrays of
// the DEVICE blob; a.v.count >= 1 and the block count fits (rviews_info_consistent).
hipError_t launch_rviews_encode(const RViewArgs &a, uint32_t k, uint32_t up, int interp, const Lut256 &lut, bool ident, hipStream_t s);

}  // namespace hgi
