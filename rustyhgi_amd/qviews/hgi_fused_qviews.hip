// Requantize view lists (hgi_qviews_requant_dev): the 128 x 64 tiles of many stored grids of different shapes, each read
// through a pitch of its own and re-coded with another quantizer table into a grid written through a pitch of its own, in ONE
// launch.
//
// Two things the companions already have, one in front of the other:
//   * "which frame am I": the view lists' search (../views/hgi_views_tile.h, view_ctx) -- a binary search of the prefix array of
//     the block's kind by scalar loads, then the frame's 64-byte record in four scalar 16-byte loads;
//   * k_requant's body (../requant/hgi_fused_requant.hip) as it stands: the encoder's LDS layout with the table at offset 0,
//     pitched_issue / stage_commit<false> / pitched_issue_odd, the cone on the source grid (cone_issue<false>, cone_finish in
//     decode mode, dec_seed_commit), dec_chain, lattice_fast, dec_fine_keep, the cone's second walk (cone_recode),
//     enc_seed_commit, enc_tile_fast / enc_tile_edge -- with W, H, the two 32-bit pitches, the two descriptors' records and the
//     frame's two pointers taken from the record where that kernel takes them from its PitchedPlan and the frame strides.
// The requantize unit is one anonymous-namespace unit and is included whole: lattice_fast, dec_fine_keep and cone_recode are
// what this unit uses; launch_requant and the four k_requant kernels come along and stay unexported (DESIGN.md 4.20 says what
// that costs).  Buffer path only: the plan refuses a list with an entry whose offsets need 64 bits, the entry point refuses the
// identity table (no kernel is instantiated for it).
// This unit defines no device function and has no store of its own: every store is the encoder tile's.
#include "../requant/hgi_fused_requant.hip"   // the encode direction's unit, the pitched staging, the tile layer, requantize's passes
#include "../views/hgi_views_tile.h"
#include "hgi_qviews_kernels.h"

namespace hgi {
namespace {

// One block (= one wave) per tile of the list.  SEEDED: 0 = the pyramid fits the tile (k = levels <= 5); 2 = the cone on the
// source grid (k == 4, sd.up = levels - 4 levels above the tile).  The wave budget is k_requant's.
template <int INTERP, int SEEDED>
__global__ __launch_bounds__(NL) __attribute__((amdgpu_waves_per_eu(HGI_ENC_WAVES_PER_EU))) void k_requant_views(
    ViewArgs a, u32 k, Lut256 lut, Seeds sd)
{
    extern __shared__ __attribute__((aligned(16))) u8 smem[];
    const int nh = k >= 2 ? (int)k : 1;
    // the encoder's layout: the table at LDS offset 0 (lut_at(); launch_tile_kernel checks on the host that there is no static LDS)
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
    // 32-bit buffer offsets on both sides (the plan serves nothing else)
    u32 rb;
    TileCtx cur = {tl, pitched_buf(fr, out, p, tl, &rb)};
    Stage st;
    if (!vc.edge) {
        pitched_issue<false>(st, cur.b.rs, rb, p.sp32, W, tl, (int)k, nh);
        if (SEEDED == 2) cone = cone_issue<false>(fr, W, H, sd, tl, at);
        lutv = lut.w[HGI_LANE];
        stage_commit<false>(buf, nullptr, st, nh);
        reinterpret_cast<u32 *>(slut)[HGI_LANE] = lutv;
        LDS_ORDER();
        pitched_issue_odd(st, cur.b.rs, rb, p.sp32);
        if (SEEDED == 2) {
            seeds = cone_finish<INTERP, false, true>(cone, buf, nullptr, sd.up, nullptr);
            LDS_ORDER();
            dec_seed_commit(buf, seeds, k);
        }
        dec_chain<INTERP, 0>(buf, tl, k, W, H);
        lattice_fast(buf, rbuf, nh);
        dec_fine_keep<INTERP>(buf, st.o);
        LDS_ORDER();
        if (SEEDED == 2) seeds = cone_recode<INTERP>(cone, buf, rbuf, sd.up, slut);
        enc_seed_commit<SEEDED>(buf, rbuf, seeds, k);
        enc_tile_fast<INTERP, false>(buf, rbuf, slut, cur, st.o, k, W, H);
        return;
    }
    if (SEEDED == 2) cone = cone_issue<false>(fr, W, H, sd, tl, at);
    pitched_issue<true, true>(st, cur.b.rs, rb, p.sp32, W, tl, (int)k, nh);
    lutv = lut.w[HGI_LANE];
    stage_commit<false>(buf, nullptr, st, nh);
    reinterpret_cast<u32 *>(slut)[HGI_LANE] = lutv;
    LDS_ORDER();
    if (SEEDED == 2) {
        seeds = cone_finish<INTERP, false, true>(cone, buf, nullptr, sd.up, nullptr);
        LDS_ORDER();
        dec_seed_commit(buf, seeds, k);
    }
    const int rows = (int)(H - tl.Y0), cols = (int)(W - tl.X0);
    if (tl.X0 + TW <= W && !(H & 1u)) {
        dec_chain<INTERP, 1>(buf, tl, k, W, H);
        lattice_fast(buf, rbuf, nh);
        dec_fine_keep<INTERP, 1>(buf, st.o, rows, cols);
        LDS_ORDER();
        if (SEEDED == 2) seeds = cone_recode<INTERP>(cone, buf, rbuf, sd.up, slut);
        enc_seed_commit<SEEDED>(buf, rbuf, seeds, k);
        enc_tile_edge<INTERP, false, 1>(buf, rbuf, slut, cur, st.o, k, W, H);
    } else {
        dec_chain<INTERP, 2>(buf, tl, k, W, H);
        lattice_fast(buf, rbuf, nh);
        dec_fine_keep<INTERP, 2>(buf, st.o, rows, cols);
        LDS_ORDER();
        if (SEEDED == 2) seeds = cone_recode<INTERP>(cone, buf, rbuf, sd.up, slut);
        enc_seed_commit<SEEDED>(buf, rbuf, seeds, k);
        enc_tile_edge<INTERP, false, 2>(buf, rbuf, slut, cur, st.o, k, W, H);
    }
}

}  // namespace

hipError_t launch_qviews_requant(const ViewArgs &a, uint32_t k, uint32_t up, int interp, const Lut256 &lut, hipStream_t s)
{
    const TileLaunch t = views_tile_launch(a, k, up);
    if (!t.ok) return hipErrorInvalidValue;
    return with_choices(
        [&](auto I, auto SE) { return launch_tile_kernel<k_requant_views<I, SE>>(t.blocks, enc_lds_bytes(t.nh), s, a, k, lut, t.sd); },
        interp_choice(interp), OneOf<2, 0>{t.cone ? 2 : 0});
}

}  // namespace hgi
