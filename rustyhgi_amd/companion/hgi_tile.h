// What the kernel units of the companion libraries (../recon, ../map, ../typed, ../requant) share on the device and in their
// launchers, on top of the tile procedure they include from ../csrc: the encoder's dynamic LDS, a plan's extra side as a tile
// sees it, the decoder's level chain without its finest pass, that pass's arithmetic, and the launch -- argument test,
// static-LDS check, the step from run-time choices to a kernel's template arguments.  A unit includes this
// behind ../csrc/hgi_fused_{enc,dec}.hip and ../csrc/hgi_fused_pitched.h.  Everything here is inlined into the unit: each
// library keeps a copy of its own, and a kernel compiles to the instructions it had when its unit spelled these out
// (profiles/r20_isa_diff.txt).
#pragma once
#include <type_traits>

#include "hgi_entry.h"
#include "hgi_sides.h"

namespace hgi {
namespace {

// ---- the encoder's LDS layout (k_enc_tiles'): the table at offset 0 (lut_at()), 256 bytes; `buf` behind it; `rbuf` behind
// that, from the next multiple of 16.  Its dynamic LDS is the uniform encoder's, nothing added.  The three pointers stay spelled
// out in each kernel: taken from a function, whatever its form, the address arithmetic is folded in another order and the
// scheduler moves instructions of the kernels (profiles/r20_companion_kernels.md).
inline size_t enc_lds_bytes(int nh) { return (size_t)buf_bytes(nh) + ((rbuf_bytes(nh) + 15) & ~15) + 256; }

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

// ---- the decoder's levels sub = 2^(k-1) ... 2 of a tile, in place: dec_tile_fast / dec_tile_edge's chain without its finest
// pass.  EDGE == 0: the tile body lies inside the image; 1: full width inside, even height; 2: any ragged tile.
template <int INTERP, int EDGE>
__device__ __forceinline__ void dec_chain(u8 *buf, Tile tl, u32 k, u32 W, u32 H)
{
    const int rows = (int)(H - tl.Y0), cols = (int)(W - tl.X0);
#define HGI_DEC_CHAIN_COARSE(SUB)                              \
    if (k > HGI_LOG2(SUB)) {                                   \
        dec_cells<INTERP, EDGE != 0>(buf, SUB, tl, W, H);      \
        dec_halo_cells<INTERP>(buf, SUB, tl, W, H);            \
        LDS_ORDER();                                           \
    }
    if (MAXK >= 6) HGI_DEC_CHAIN_COARSE(32)
    if (MAXK >= 5) HGI_DEC_CHAIN_COARSE(16)
    HGI_DEC_CHAIN_COARSE(8)
    HGI_DEC_CHAIN_COARSE(4)
#undef HGI_DEC_CHAIN_COARSE
    if (k >= 2) {
        dec_level2_fast<INTERP, EDGE>(buf, rows, cols);
        dec_halo_cells<INTERP>(buf, 2, tl, W, H);
        LDS_ORDER();
    }
}

// ---- the arithmetic of the decoder's finest pass (dec_fine_fast's) on one task of a lane: E, F the lattice rows above and below
// as loaded, e16 / f16 their ninth corners, O the residuals of row y + 1.  Out come row y (E with its odd columns decoded) and
// row y + 1.  The loads and the choice of the ninth corner stay with the caller: moved in here too, the scheduler orders them
// differently in the Crossed kernels.
template <int INTERP>
__device__ __forceinline__ void dec_fine_rows(v4u E, v4u F, u32 e16, u32 f16, v4u O, v4u &r0v, v4u &r1v)
{
    uint2 c, fl;
    c.x = __builtin_amdgcn_perm(E.y, E.x, 0x06040200u);
    c.y = __builtin_amdgcn_perm(E.w, E.z, 0x06040200u);
    fl.x = __builtin_amdgcn_perm(F.y, F.x, 0x06040200u);
    fl.y = __builtin_amdgcn_perm(F.w, F.z, 0x06040200u);
    u32 P0, P1;
    pred8<INTERP>(c, e16, fl, f16, P0, P1);
    u32 e0 = E.x, e1 = E.y, e2 = E.z, e3 = E.w, o0 = O.x, o1 = O.y, o2 = O.z, o3 = O.w;
    // row y: odd columns;  cell j of the lane = byte j of P0 (j < 4) or byte j-4 of P1
    HGI_ADDB(e0, 1, P0, 0); HGI_ADDB(e0, 3, P0, 1); HGI_ADDB(e1, 1, P0, 2); HGI_ADDB(e1, 3, P0, 3);
    HGI_ADDB(e2, 1, P1, 0); HGI_ADDB(e2, 3, P1, 1); HGI_ADDB(e3, 1, P1, 2); HGI_ADDB(e3, 3, P1, 3);
    // row y+1: every column
    HGI_ADDB(o0, 0, P0, 0); HGI_ADDB(o0, 1, P0, 0); HGI_ADDB(o0, 2, P0, 1); HGI_ADDB(o0, 3, P0, 1);
    HGI_ADDB(o1, 0, P0, 2); HGI_ADDB(o1, 1, P0, 2); HGI_ADDB(o1, 2, P0, 3); HGI_ADDB(o1, 3, P0, 3);
    HGI_ADDB(o2, 0, P1, 0); HGI_ADDB(o2, 1, P1, 0); HGI_ADDB(o2, 2, P1, 1); HGI_ADDB(o2, 3, P1, 1);
    HGI_ADDB(o3, 0, P1, 2); HGI_ADDB(o3, 1, P1, 2); HGI_ADDB(o3, 2, P1, 3); HGI_ADDB(o3, 3, P1, 3);
    r0v = v4u{e0, e1, e2, e3};
    r1v = v4u{o0, o1, o2, o3};
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

// One kernel, one wave per block: the tables are addressed from LDS offset 0, so that the compiler placed no static LDS in
// front of them is checked on the host, once per instantiation; then the launch and its error.
template <auto K, class... A>
hipError_t launch_tile_kernel(const TileLaunch &t, size_t lds, hipStream_t s, const A &...args)      // (the table is 256 bytes)
{
    static const hipError_t lds0 = static_lds_is_empty(reinterpret_cast<const void *>(K));
    if (lds0 != hipSuccess) return lds0;
    hipLaunchKernelGGL(K, t.blocks, dim3(NL), lds, s, args...);
    return hipGetLastError();
}

// Run-time choices to template arguments: with_choices(f, OneOf<A...>{a}, OneOf<B...>{b}, ...) calls f(Const<a>{}, Const<b>{},
// ...), whose parameters a generic lambda can name as a kernel's template arguments.  A value that is none of its list ends
// the call with hipErrorInvalidValue.  Only the listed combinations are instantiated, in the order of the lists, the last
// choice running fastest -- and that is the order of the kernels in the unit's code object, which is not free: listed the
// other way round, typed encode's E = 4 kernels come out with other registers (profiles/r20_companion_kernels.md).
template <int V>
using Const = std::integral_constant<int, V>;
template <int... V>
struct OneOf {
    int v;
};

template <class F, int V, class... C>
hipError_t with_choices(const F &f, Const<V> c0, C... c)      // every choice made: they stand in the order given
{
    return f(c0, c...);
}

template <class F, int V0, int... V, class... C>
hipError_t with_choices(const F &f, OneOf<V0, V...> o, C... c)      // the first open choice moves behind the others as a constant
{
    if (o.v == V0) return with_choices(f, c..., Const<V0>{});
    if constexpr (sizeof...(V) > 0) return with_choices(f, OneOf<V...>{o.v}, c...);
    return hipErrorInvalidValue;
}

}  // namespace
}  // namespace hgi
