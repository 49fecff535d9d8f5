// The decoder's level chain without its finest pass: what a decoder that brings a finest level of its own (region decode's
// clipped store; the companions' mapped and requantizing ones) takes from the decode tile procedure beside dec_fine_rows.
// Device code; included behind hgi_fused_dec.hip, whose dec_cells, dec_halo_cells and dec_level2_fast it calls.  A kernel that
// calls it compiles to the instructions it had when its unit spelled the chain out (profiles/r20_isa_diff.txt,
// r22_isa_diff.txt); dec_tile_edge of hgi_fused_impl.h does not -- the uniform, 16-row and pitched decoders change -- and keeps
// its own (profiles/r22_launch_layer.md).
#pragma once

namespace hgi {
namespace {

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

}  // namespace
}  // namespace hgi
