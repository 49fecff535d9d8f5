// Internal launch interface between hgi_map.hip (entry points, argument checks, plan) and hgi_fused_map_dec.hip (kernels).
#pragma once
#include "../csrc/hgi_kernels.h"
#include "hgi_map_plan.h"

namespace hgi {

// One launch: the tiles of every frame, k fused levels (1 ... kFusedMaxLevels) and, with up >= 1 (k == 4 only), the cone that
// rebuilds the `up` <= 4 levels above a tile from the frame's own samples.  `table`: 256 elements of `elem` (2 or 4) bytes in
// device memory.  mp.p.fast and mp.p.ok must hold.
hipError_t launch_decode_map(const uint8_t *grid, const void *table, void *out, const MapPlan &mp, uint32_t elem, uint32_t k,
                             uint32_t up, int interp, hipStream_t s);

}  // namespace hgi
