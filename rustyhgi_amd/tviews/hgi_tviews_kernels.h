// Internal launch interface between hgi_tviews.hip (entry points, argument checks, plan) and hgi_fused_tviews_enc.hip (kernels).
#pragma once
#include "../csrc/hgi_kernels.h"
#include "hgi_tviews_plan.h"

namespace hgi {

// One launch: the tiles of every frame of the list, k fused levels (1 ... kFusedMaxLevels) and, with up >= 1 (k == 4 only), the
// cone that rebuilds the `up` <= 4 levels above a tile from the frame's own samples through its byte pitch.  a: the arrays of
// the DEVICE blob; a.count >= 1 and the block count fits (tviews_info_consistent).  The frames hold elements of `elem` bytes,
// IEEE (float16 at 2, float32 at 4) or, with `bf16` (elem 2 only), bfloat16; the pixel of element x is
// clamp(rint(x * scale + bias), 0, 255), 0 for NaN (include/hgi_typed.h).
hipError_t launch_tviews_encode(const ViewArgs &a, uint32_t elem, bool bf16, float scale, float bias, uint32_t k, uint32_t up, int interp,
                                const Lut256 &lut, bool ident, hipStream_t s);

}  // namespace hgi
