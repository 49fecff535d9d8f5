// Internal launch interface between hgi_recon.hip (entry points, argument checks, plan) and hgi_fused_recon_enc.hip (kernels).
#pragma once
#include "../csrc/hgi_kernels.h"
#include "hgi_recon_plan.h"

namespace hgi {

// One launch: the tiles of every frame, k fused levels (1 ... kFusedMaxLevels) and, with up >= 1 (k == 4 only), the cone that
// rebuilds the `up` <= 4 levels above a tile from the frame's own samples.  rp.p.fast and rp.p.ok must hold.
hipError_t launch_encode_recon(const uint8_t *img, uint8_t *grid, uint8_t *recon, const ReconPlan &rp, uint32_t k, uint32_t up,
                               int interp, const Lut256 &lut, bool ident, hipStream_t s);

}  // namespace hgi
