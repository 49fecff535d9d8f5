// Device side of the frame lists, shared by hgi_fused_list_dec.hip and hgi_fused_list_enc.hip (each includes it after its
// direction's unit): how a block finds its frame and its tile (hgi_framelist.h holds the plan and the map itself).
#pragma once
#include "hgi_framelist.h"

namespace hgi {
namespace {

static_assert(TW == (int)kListTileW && TH == (int)kListTileH, "the list plan is laid out on 128 x 64 tiles");

// The table is read through the constant address space: every index is wave-uniform (a function of blockIdx), so each probe
// of the search and the frame's 64-byte record are scalar loads.  Device code never writes the table.
typedef __attribute__((address_space(4))) const u32 list_cu32;
typedef __attribute__((address_space(4))) const v4u list_cv4;

// What a list block starts from: its frame's record and its tile.
struct ListTileCtx {
    bool edge, idle;
    Tile tl;
    const u8 *fr;
    u8 *out;
    u32 W, H, aligned;
};

__device__ __forceinline__ ListTileCtx list_ctx(const ListArgs &a)
{
    // the launch constants at the kernel's first instruction, in one go (args_early's reasoning); the search behind them is
    // log2(count) dependent scalar loads
#if HGI_ARGS_EARLY
    asm volatile("" ::"s"(a.frames), "s"(a.epre), "s"(a.ipre), "s"(a.count), "s"(a.nedge), "s"(a.nint));
#endif
    ListTileCtx c;
    ListBlock r = list_role(blockIdx.x, a.nedge, a.nint);
    c.edge = r.edge;
    c.idle = r.idle;
    if (r.idle) return c;
    list_cu32 *pre = (list_cu32 *)(r.edge ? a.epre : a.ipre);
    r.frame = list_find(pre, a.count, r.t);
    list_cv4 *rec = (list_cv4 *)a.frames + 4u * r.frame;
    const v4u words[4] = {rec[0], rec[1], rec[2], rec[3]};
    ListFrame F;
    __builtin_memcpy(&F, words, sizeof(F));
    list_tile(r, F, pre[r.frame]);
    c.tl.frame = 0;      // (the record holds the frame's pointers: no frame stride, no seed planes)
    c.tl.X0 = r.tx * TW;
    c.tl.Y0 = r.ty * TH;
    c.fr = reinterpret_cast<const u8 *>(F.src);
    c.out = reinterpret_cast<u8 *>(F.dst);
    c.W = F.width;
    c.H = F.height;
    c.aligned = F.aligned;
    return c;
}

}  // namespace
}  // namespace hgi
