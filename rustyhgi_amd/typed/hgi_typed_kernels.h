// Internal launch interface between hgi_typed.hip (entry point, argument checks, plan) and hgi_fused_typed_enc.hip (kernels).
#pragma once
#include "../csrc/hgi_kernels.h"
#include "hgi_typed_plan.h"

namespace hgi {

// One launch: the tiles of every frame, k fused levels (1 ... kFusedMaxLevels) and, with up >= 1 (k == 4 only), the cone that
// rebuilds the `up` <= 4 levels above a tile from the frame's own samples.  `img`: elements of `elem` bytes, IEEE (float16 at
// 2, float32 at 4) or, with `bf16` (elem 2 only), bfloat16; the pixel of element x is clamp(rint(x * scale + bias), 0, 255),
// 0 for NaN (include/hgi_typed.h).  tp.p.fast and tp.p.ok must hold.
hipError_t launch_encode_typed(const void *img, uint8_t *grid, const TypedPlan &tp, uint32_t elem, bool bf16, float scale, float bias,
                               uint32_t k, uint32_t up, int interp, const Lut256 &lut, bool ident, hipStream_t s);

}  // namespace hgi
