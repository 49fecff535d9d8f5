// View-list encode (hgi_views_encode_dev): the 128 x 64 tiles of many images of different shapes, each with a read pitch and a
// write pitch of its own, in ONE launch.  The decode unit (hgi_fused_views_dec.hip) says how a block finds its frame and what it
// takes from the frame's record; each tile then runs k_enc_pitched's fast path as it stands: the table at LDS offset 0, the cone
// through the read pitch, enc_tile_fast / enc_tile_edge.  This is the 64-row build of the encoder; a 32-row one is not built.
#define HGI_FUSED_NO_LAUNCHERS 1
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"
#pragma clang diagnostic ignored "-Wunneeded-internal-declaration"
#include "../csrc/hgi_fused_enc.hip"   // the encode direction's build settings and tile procedure, 128 x 64 tiles
#include "../csrc/hgi_fused_pitched.h"
#pragma clang diagnostic pop
#include "../companion/hgi_tile.h"
#include "hgi_views_tile.h"

namespace hgi {
namespace {

// SEEDED: as in k_dec_views.  The wave budget is k_enc_pitched's.
template <int INTERP, bool IDENT, int SEEDED>
__global__ __launch_bounds__(NL) __attribute__((amdgpu_waves_per_eu(IDENT ? HGI_ENC_WAVES_PER_EU - 1 : HGI_ENC_WAVES_PER_EU))) void k_enc_views(
    ViewArgs a, u32 k, Lut256 lut, Seeds sd)
{
    extern __shared__ __attribute__((aligned(16))) u8 smem[];
    const int nh = k >= 2 ? (int)k : 1;
    // the table at LDS offset 0 (lut_at(); launch_tile_kernel checks on the host that there is no static LDS)
    u8 *slut = smem;
    u8 *buf = smem + 256 - HCOL;
    u8 *rbuf = smem + 256 + buf_bytes(nh) - RCOL;
    const ViewTileCtx vc = view_ctx(a);
    if (vc.idle) return;
    const Tile tl = vc.tl;
    const PitchedPlan &p = vc.p;
    const u32 W = p.W, H = p.H;
    const u8 *fr = vc.fr;
    u8 *out = vc.out;
    const PitchAt at = {p.sp};
    u32 lutv = 0;
    SeedRegs seeds;
    ConeLane cone;
    u32 rb;
    TileCtx cur = {tl, pitched_buf(fr, out, p, tl, &rb)};
    Stage st;
    if (!vc.edge) {
        pitched_issue<false>(st, cur.b.rs, rb, p.sp32, W, tl, (int)k, nh);
        if (SEEDED == 2) cone = cone_issue<true>(fr, W, H, sd, tl, at);
        if (!IDENT) lutv = lut.w[HGI_LANE];
        stage_commit<true>(buf, rbuf, st, nh);
        if (!IDENT) reinterpret_cast<u32 *>(slut)[HGI_LANE] = lutv;
        LDS_ORDER();
        pitched_issue_odd(st, cur.b.rs, rb, p.sp32);
        if (SEEDED == 2) seeds = cone_finish<INTERP, true, IDENT>(cone, buf, rbuf, sd.up, slut);
        enc_seed_commit<SEEDED>(buf, rbuf, seeds, k);
        enc_tile_fast<INTERP, IDENT>(buf, rbuf, slut, cur, st.o, k, W, H);
        return;
    }
    if (SEEDED == 2) cone = cone_issue<true>(fr, W, H, sd, tl, at);
    pitched_issue<true, true>(st, cur.b.rs, rb, p.sp32, W, tl, (int)k, nh);
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
}

}  // namespace

hipError_t launch_views_encode(const ViewArgs &a, uint32_t k, uint32_t up, int interp, const Lut256 &lut, bool ident, hipStream_t s)
{
    const TileLaunch t = views_tile_launch(a, k, up);
    if (!t.ok) return hipErrorInvalidValue;
    return with_choices(
        [&](auto I, auto ID, auto SE) { return launch_tile_kernel<k_enc_views<I, ID != 0, SE>>(t.blocks, enc_lds_bytes(t.nh), s, a, k, lut, t.sd); },
        interp_choice(interp), OneOf<1, 0>{ident ? 1 : 0}, OneOf<2, 0>{t.cone ? 2 : 0});
}

}  // namespace hgi
