// What the kernel units of the companion libraries (../recon, ../map, ../typed, ../requant, ../views) share on top of what they
// include from ../csrc -- the tile procedure, the launch layer (hgi_launch.h: the encoder's dynamic LDS, the static-LDS check,
// with_choices, launch_tile_kernel) and the decoder's level chain without its finest pass (hgi_dec_chain.h): a plan's extra side
// as a tile sees it, and what a launcher works out first.  A unit includes this behind
// ../csrc/hgi_fused_{enc,dec}.hip and ../csrc/hgi_fused_pitched.h.  Everything here is inlined into the unit: each library keeps
// a copy of its own.
#pragma once
#include "../csrc/hgi_dec_chain.h"
#include "../csrc/hgi_launch.h"
#include "hgi_entry.h"
#include "hgi_sides.h"

namespace hgi {
namespace {

// ---- a plan's extra side (hgi_sides.h, ExtraSide) at one tile: Buf's descriptor, `W` and `base` once more ----------------------
struct TileSide {
    __amdgpu_buffer_rsrc_t r;      // over one frame's records
    u32 pitch, base;               // bytes between rows, Y0 * pitch + X0 * E
};

// `fr`: the frame's first byte; `elem`: bytes per element of the side
__device__ __forceinline__ TileSide tile_side(const ExtraSide &x, const u8 *fr, Tile tl, u32 elem)
{
    TileSide t;
    t.r = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(fr), 0, x.rec, 0x00020000);
    t.pitch = x.pitch32;
    t.base = __builtin_amdgcn_readfirstlane(tl.Y0 * x.pitch32 + tl.X0 * elem);
    return t;
}

// ---- the launch ------------------------------------------------------------------------------------------------------------
// What every launcher works out first: whether the call is one the kernels serve (k fused levels of a fast plan; a cone only
// over four levels and of at most kConeMaxUp), the cone's argument, the halo depth and the grid of one block per tile.
struct TileLaunch {
    bool ok, cone;
    Seeds sd;
    int nh;
    dim3 blocks;
};

inline TileLaunch tile_launch(const PitchedPlan &p, u32 k, u32 up)
{
    TileLaunch t = {};
    t.cone = up != 0;
    t.ok = k >= 1 && k <= (u32)MAXK && p.ok && p.fast && !(t.cone && (k != 4 || up > (u32)kConeMaxUp));
    t.sd = Seeds{nullptr, nullptr, 0, 0, 0, up};
    t.nh = k >= 2 ? (int)k : 1;
    t.blocks = dim3((u32)pitched_blocks(p));
    return t;
}

}  // namespace
}  // namespace hgi
