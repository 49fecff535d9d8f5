// Internal launch interface between hgi_sviews.hip (entry points, argument checks, plan) and hgi_fused_sviews_dec.hip (kernels).
#pragma once
#include "../csrc/hgi_kernels.h"
#include "hgi_sviews_plan.h"

namespace hgi {

// One launch: the tiles of every output image of the list, k fused levels (1 ... 5) of the levels - shift that remain and, with
// up >= 1 (k == 4 only), the cone that rebuilds the `up` <= 4 levels above a tile from the grid's own lattice samples through its
// read pitch.  a: the arrays of the DEVICE blob; a.count >= 1 and the block count fits (sviews_info_consistent).  max_width: the
// widest output image (the decoder's occupancy policy).  shift: 1 ... 31, the one the plan was made for.
hipError_t launch_sviews_decode(const ViewArgs &a, uint32_t max_width, uint32_t shift, uint32_t k, uint32_t up, int interp, hipStream_t s);

}  // namespace hgi
