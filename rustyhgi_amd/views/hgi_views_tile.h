// Device side of the view lists, shared by hgi_fused_views_dec.hip and hgi_fused_views_enc.hip (each includes it behind its
// direction's unit, ../csrc/hgi_fused_pitched.h and ../companion/hgi_tile.h): how a block finds its frame and its tile -- the
// frame lists' search (csrc/hgi_fused_list.h, list_ctx) on this library's record -- and what the pitched staging takes from
// that record where the pitched kernels take it from their PitchedPlan.
#pragma once
#include "hgi_views_kernels.h"

namespace hgi {
namespace {

static_assert(TW == (int)kListTileW && TH == (int)kListTileH, "the plan is laid out on 128 x 64 tiles");

// The blob is read through the constant address space: every index is wave-uniform (a function of blockIdx), so each probe of
// the search and the frame's 64-byte record are scalar loads.  Device code never writes the blob.
typedef __attribute__((address_space(4))) const u32 view_cu32;
typedef __attribute__((address_space(4))) const v4u view_cv4;

// What a block starts from: its tile, and its frame's record as the part of a PitchedPlan the fast path reads (W, H, the two
// 32-bit pitches, the two record counts; sp for the cone's addressing) with the frame's two pointers.
struct ViewTileCtx {
    bool edge, idle;
    Tile tl;
    const u8 *fr;
    u8 *out;
    PitchedPlan p;
};

__device__ __forceinline__ ViewTileCtx view_ctx(const ViewArgs &a)
{
    // the launch constants at the kernel's first instruction, in one go (list_ctx's reasoning); the search behind them is
    // log2(count) dependent scalar loads
#if HGI_ARGS_EARLY
    asm volatile("" ::"s"(a.frames), "s"(a.epre), "s"(a.ipre), "s"(a.count), "s"(a.nedge), "s"(a.nint));
#endif
    ViewTileCtx c;
    ListBlock r = list_role(blockIdx.x, a.nedge, a.nint);
    c.edge = r.edge;
    c.idle = r.idle;
    if (r.idle) return c;
    view_cu32 *pre = (view_cu32 *)(r.edge ? a.epre : a.ipre);
    r.frame = list_find(pre, a.count, r.t);
    view_cv4 *rec = (view_cv4 *)a.frames + 4u * r.frame;
    const v4u words[4] = {rec[0], rec[1], rec[2], rec[3]};
    ViewFrame F;
    __builtin_memcpy(&F, words, sizeof(F));
    view_tile(r, F, pre[r.frame]);
    c.tl.frame = 0;      // (the record holds the frame's pointers: no frame stride, no seed planes)
    c.tl.X0 = __builtin_amdgcn_readfirstlane(r.tx * TW);
    c.tl.Y0 = __builtin_amdgcn_readfirstlane(r.ty * TH);
    c.fr = reinterpret_cast<const u8 *>(F.src);
    c.out = reinterpret_cast<u8 *>(F.dst);
    c.p = PitchedPlan{};
    c.p.W = F.width;
    c.p.H = F.height;
    c.p.fast = 1u;
    c.p.sp32 = F.sp32;
    c.p.dp32 = F.dp32;
    c.p.srec = F.srec;
    c.p.drec = F.drec;
    c.p.sp = F.sp32;
    c.p.dp = F.dp32;
    return c;
}

// What both launchers work out first (tile_launch of ../companion/hgi_tile.h, on a list instead of a PitchedPlan).
inline TileLaunch views_tile_launch(const ViewArgs &a, u32 k, u32 up)
{
    TileLaunch t = {};
    const u64 blocks = list_blocks(a.nedge, a.nint);
    t.cone = up != 0;
    t.ok = k >= 1 && k <= (u32)MAXK && a.count != 0 && blocks != 0 && blocks + 8 < (1ull << 31) && !(t.cone && (k != 4 || up > (u32)kConeMaxUp));
    t.sd = Seeds{nullptr, nullptr, 0, 0, 0, up};
    t.nh = k >= 2 ? (int)k : 1;
    t.blocks = dim3((u32)blocks);
    return t;
}

}  // namespace
}  // namespace hgi
