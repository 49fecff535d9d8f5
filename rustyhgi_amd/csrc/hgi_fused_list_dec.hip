// Frame-list decode (hgi_decode_u8_list_dev): the 128 x 64 tiles of many frames of different shapes in ONE launch.
//
// The fused decoder codes every tile from its own frame's bytes, so a tile of frame i of a list, staged
// from the same grid bytes at the same origin, runs exactly the code a lone decode of that frame runs -- k_dec_tiles' tile
// procedure as it stands: staging, the cone, dec_tile_fast / dec_tile_edge / the byte-checked path -- on the frame's own
// width, height, grid and output.  What is new is the tile list: hgi_framelist.h (plain C++, shared with the host test) lays
// the edge tiles of all frames first and the interior tiles behind them, and a block finds its frame by a binary search over
// the prefix array of its kind, then reads the frame's record (one scalar load) and derives its tile.  The frame's geometry
// and `aligned` bits are what fused_geom computes for a batch of one, so each tile takes the path the lone decode's tile takes.
// Every pixel access goes through the frame's own buffer descriptors (make_buf: W * H records) or the byte-checked path.
#define HGI_FUSED_NO_LAUNCHERS 1
#include "hgi_fused_dec.hip"   // the decode direction's build settings and tile procedure, 128 x 64 tiles
#include "hgi_fused_list.h"

namespace hgi {
namespace {

// One block (= one wave) per tile of the list.  SEEDED: 0 = the pyramid fits the tile (k = levels <= 5); 2 = the cone (k == 4,
// sd.up = levels - 4 levels above the tile, rebuilt from the frame's own base samples).  The wave budget is k_dec_tiles'.
template <int INTERP, int SEEDED>
__global__ __launch_bounds__(NL) __attribute__((amdgpu_waves_per_eu(SEEDED == 2 ? HGI_DEC_WAVES_PER_EU - 2 : HGI_DEC_WAVES_PER_EU))) void k_dec_list(
    ListArgs a, u32 k, Seeds sd)
{
    extern __shared__ __attribute__((aligned(16))) u8 smem[];
    const int nh = k >= 2 ? (int)k : 1;
    u8 *buf = smem - HCOL;
    const ListTileCtx lc = list_ctx(a);
    if (lc.idle) return;
    const Tile tl = lc.tl;
    const u32 W = lc.W, H = lc.H;
    SeedRegs seeds;
    ConeLane cone;
    if (!lc.edge) {
        TileCtx cur = {tl, make_buf(lc.fr, lc.out, W, H, tl, (lc.aligned & 4u) ? 3u : 0u)};
        Stage st;
        stage_issue<false>(st, cur.b, tl, (int)k, nh);
        if (SEEDED == 2) cone = cone_issue<false>(lc.fr, W, H, sd, tl);
        stage_commit<false>(buf, nullptr, st, nh);
        LDS_ORDER();
        if (HGI_ODD_LATE) stage_issue_odd(st, cur.b);
        if (SEEDED == 2) seeds = cone_finish<INTERP, false, true>(cone, buf, nullptr, sd.up, nullptr);
        LDS_ORDER();
        if (SEEDED) dec_seed_commit(buf, seeds, k);
        dec_tile_fast<INTERP>(buf, cur, st.o, k, W, H);
        return;
    }
    // ragged tile (body crosses the image edge), or a frame whose byte offsets do not fit 32 bits: k_dec_tiles' edge paths
    if (SEEDED == 2) cone = cone_issue<false>(lc.fr, W, H, sd, tl);
    if (lc.aligned & 2u) {
        TileCtx cur = {tl, make_buf(lc.fr, lc.out, W, H, tl, (lc.aligned & 4u) ? 3u : 0u)};
        Stage st;
        stage_issue<true, true>(st, cur.b, tl, (int)k, nh);
        stage_commit<false>(buf, nullptr, st, nh);
        LDS_ORDER();
        if (SEEDED == 2) seeds = cone_finish<INTERP, false, true>(cone, buf, nullptr, sd.up, nullptr);
        if (SEEDED) dec_seed_commit(buf, seeds, k);
        if (tl.X0 + TW <= W && !(H & 1u))
            dec_tile_edge<INTERP, 1>(buf, cur, st.o, k, W, H);
        else
            dec_tile_edge<INTERP, 2>(buf, cur, st.o, k, W, H);
        return;
    }
    stage_tile_generic(buf, lc.fr, W, H, tl, nh, (lc.aligned & 1u) != 0);
    LDS_ORDER();
    if (SEEDED == 2) seeds = cone_finish<INTERP, false, true>(cone, buf, nullptr, sd.up, nullptr);
    if (SEEDED) dec_seed_commit(buf, seeds, k);
    for (int s = 1 << (k - 1); s >= 2; s >>= 1) {
        dec_cells<INTERP, true>(buf, s, tl, W, H);
        dec_halo_cells<INTERP>(buf, s, tl, W, H);
        LDS_ORDER();
    }
    dec_fine_generic<INTERP>(buf, lc.fr, lc.out, tl, W, H, (lc.aligned & 1u) != 0);
}

}  // namespace

hipError_t launch_decode_list(const ListArgs &a, uint32_t max_width, uint32_t k, int interp, const Seeds *seeds, hipStream_t s)
{
    if (k < 1 || k > (u32)MAXK || a.count == 0) return hipErrorInvalidValue;
    const u64 blocks = list_blocks(a.nedge, a.nint);
    if (blocks == 0 || blocks + 8 >= (1ull << 31)) return hipErrorInvalidValue;
    const bool cone = seeds && seeds->up != 0;
    if (seeds && (!cone || k != 4 || seeds->up > (u32)kConeMaxUp || seeds->rec)) return hipErrorInvalidValue;   // (the cone on the frame's own samples only)
    const Seeds sd = seeds ? *seeds : Seeds{nullptr, nullptr, 0, 0, 0, 0};
    const int nh = k >= 2 ? (int)k : 1;
    // resident tiles per CU: on the list's tile count and its widest frame
    const size_t lds = lds_for_waves((size_t)buf_bytes(nh), dec_resident_tiles((u64)a.nedge + a.nint, max_width, k, seeds != nullptr));
    return with_choices([&](auto I, auto SE) { return launch_tile_kernel<k_dec_list<I, SE>>(dim3((u32)blocks), lds, s, a, k, sd); },
                        interp_choice(interp), OneOf<2, 0>{cone ? 2 : 0});
}

}  // namespace hgi
