// Frame-list encode (hgi_encode_u8_list_dev): the 128 x 64 tiles of many frames of different shapes in ONE launch.
// The decode unit (hgi_fused_list_dec.hip) says how a block finds its frame and tile; each tile then runs k_enc_tiles' tile
// procedure as it stands -- staging, the table in LDS, the cone, enc_tile_fast / enc_tile_edge / the byte-checked path -- on
// the frame's own width, height, image and grid.  This is the 64-row build of the encoder; the uniform plain encode runs
// 32-row tiles on most calls (hgi_capi.hip use_tile_rows), and a 32-row list encoder is not built.
#define HGI_FUSED_NO_LAUNCHERS 1
#include "hgi_fused_enc.hip"   // the encode direction's build settings and tile procedure, 128 x 64 tiles
#include "hgi_fused_list.h"

namespace hgi {
namespace {

// SEEDED: as in k_dec_list.  The wave budget is k_enc_tiles'.
template <int INTERP, bool IDENT, int SEEDED>
__global__ __launch_bounds__(NL) __attribute__((amdgpu_waves_per_eu(IDENT ? HGI_ENC_WAVES_PER_EU - 1 : HGI_ENC_WAVES_PER_EU))) void k_enc_list(
    ListArgs a, u32 k, Lut256 lut, Seeds sd)
{
    extern __shared__ __attribute__((aligned(16))) u8 smem[];
    const int nh = k >= 2 ? (int)k : 1;
    // the table at LDS offset 0 (lut_at(); launch_encode_list checks on the host that there is no static LDS)
    u8 *slut = smem;
    u8 *buf = smem + 256 - HCOL;
    u8 *rbuf = smem + 256 + buf_bytes(nh) - RCOL;
    const ListTileCtx lc = list_ctx(a);
    if (lc.idle) return;
    const Tile tl = lc.tl;
    const u32 W = lc.W, H = lc.H;
    u32 lutv = 0;
    SeedRegs seeds;
    ConeLane cone;
    if (!lc.edge) {
        TileCtx cur = {tl, make_buf(lc.fr, lc.out, W, H, tl, (lc.aligned & 4u) ? 3u : 0u)};
        Stage st;
        stage_issue<false>(st, cur.b, tl, (int)k, nh);
        if (SEEDED == 2) cone = cone_issue<true>(lc.fr, W, H, sd, tl);
        if (!IDENT) lutv = lut.w[HGI_LANE];
        stage_commit<true>(buf, rbuf, st, nh);
        if (!IDENT) reinterpret_cast<u32 *>(slut)[HGI_LANE] = lutv;
        LDS_ORDER();
        if (HGI_ODD_LATE) stage_issue_odd(st, cur.b);
        if (SEEDED == 2) seeds = cone_finish<INTERP, true, IDENT>(cone, buf, rbuf, sd.up, slut);
        enc_seed_commit<SEEDED>(buf, rbuf, seeds, k);
        enc_tile_fast<INTERP, IDENT>(buf, rbuf, slut, cur, st.o, k, W, H);
        return;
    }
    if (SEEDED == 2) cone = cone_issue<true>(lc.fr, W, H, sd, tl);
    if (lc.aligned & 2u) {
        TileCtx cur = {tl, make_buf(lc.fr, lc.out, W, H, tl, (lc.aligned & 4u) ? 3u : 0u)};
        Stage st;
        stage_issue<true, true>(st, cur.b, tl, (int)k, nh);
        if (!IDENT) lutv = lut.w[HGI_LANE];
        stage_commit<true>(buf, rbuf, st, nh);
        if (!IDENT) reinterpret_cast<u32 *>(slut)[HGI_LANE] = lutv;
        LDS_ORDER();
        if (SEEDED == 2) seeds = cone_finish<INTERP, true, IDENT>(cone, buf, rbuf, sd.up, slut);
        enc_seed_commit<SEEDED>(buf, rbuf, seeds, k);
        if (tl.X0 + TW <= W && !(H & 1u))
            enc_tile_edge<INTERP, IDENT, 1>(buf, rbuf, slut, cur, st.o, k, W, H);
        else
            enc_tile_edge<INTERP, IDENT, 2>(buf, rbuf, slut, cur, st.o, k, W, H);
        return;
    }
    if (!IDENT) reinterpret_cast<u32 *>(slut)[HGI_LANE] = lut.w[HGI_LANE];
    stage_tile_generic(buf, lc.fr, W, H, tl, nh, (lc.aligned & 1u) != 0);
    LDS_ORDER();
    lattice_from_buf(buf, rbuf, nh);
    LDS_ORDER();
    if (SEEDED == 2) seeds = cone_finish<INTERP, true, IDENT>(cone, buf, rbuf, sd.up, slut);
    enc_seed_commit<SEEDED>(buf, rbuf, seeds, k);
    for (int s = 1 << (k - 1); s >= 2; s >>= 1) {
        enc_cells<INTERP, IDENT, true>(buf, rbuf, slut, s, tl, W, H);
        enc_halo_pass<INTERP, IDENT>(buf, rbuf, slut, s, tl, W, H);
        LDS_ORDER();
    }
    enc_fine_generic<INTERP, IDENT>(buf, rbuf, slut, lc.fr, lc.out, tl, W, H, (lc.aligned & 1u) != 0);
}

}  // namespace

hipError_t launch_encode_list(const ListArgs &a, uint32_t k, int interp, const Lut256 &lut, bool ident, const Seeds *seeds, hipStream_t s)
{
    if (k < 1 || k > (u32)MAXK || a.count == 0) return hipErrorInvalidValue;
    const u64 blocks = list_blocks(a.nedge, a.nint);
    if (blocks == 0 || blocks + 8 >= (1ull << 31)) return hipErrorInvalidValue;
    const bool cone = seeds && seeds->up != 0;
    if (seeds && (!cone || k != 4 || seeds->up > (u32)kConeMaxUp || seeds->rec || seeds->q)) return hipErrorInvalidValue;
    const Seeds sd = seeds ? *seeds : Seeds{nullptr, nullptr, 0, 0, 0, 0};
    const int nh = k >= 2 ? (int)k : 1;
    const size_t lds = lds_for_waves(enc_lds_bytes(nh), HGI_KNOB(HGI_ENC_WAVES, 0));
    return with_choices(
        [&](auto I, auto ID, auto SE) { return launch_tile_kernel<k_enc_list<I, ID != 0, SE>>(dim3((u32)blocks), lds, s, a, k, lut, sd); },
        interp_choice(interp), OneOf<1, 0>{ident ? 1 : 0}, OneOf<2, 0>{cone ? 2 : 0});
}

}  // namespace hgi
