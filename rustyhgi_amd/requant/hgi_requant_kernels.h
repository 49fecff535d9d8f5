// Internal launch interface between hgi_requant.hip (entry points, argument checks, plan) and hgi_fused_requant.hip (kernels).
#pragma once
#include "../csrc/hgi_kernels.h"
#include "hgi_requant_plan.h"

namespace hgi {

// One launch: the tiles of every frame, k fused levels (1 ... kFusedMaxLevels) in both directions and, with up >= 1 (k == 4
// only), the cone that rebuilds the `up` <= 4 levels above a tile from the source grid.  p.fast and p.ok must hold; the table
// is not the identity.
hipError_t launch_requant(const uint8_t *src, uint8_t *dst, const PitchedPlan &p, uint32_t k, uint32_t up, int interp,
                          const Lut256 &lut, hipStream_t s);

}  // namespace hgi
