// Internal launch interface between hgi_views.hip (entry points, argument checks, plan) and the two kernel units,
// hgi_fused_views_dec.hip and hgi_fused_views_enc.hip.
#pragma once
#include "../csrc/hgi_kernels.h"
#include "hgi_views_plan.h"

namespace hgi {

// One launch each: the tiles of every frame of the list, k fused levels (1 ... kFusedMaxLevels) and, with up >= 1 (k == 4
// only), the cone that rebuilds the `up` <= 4 levels above a tile from the frame's own samples through its read pitch.
// a: the arrays of the DEVICE blob; a.count >= 1 and the block count fits (views_info_consistent).  max_width: the widest frame
// (the decoder's occupancy policy).
hipError_t launch_views_decode(const ViewArgs &a, uint32_t max_width, uint32_t k, uint32_t up, int interp, hipStream_t s);
hipError_t launch_views_encode(const ViewArgs &a, uint32_t k, uint32_t up, int interp, const Lut256 &lut, bool ident, hipStream_t s);

}  // namespace hgi
