// View-list decode (hgi_views_decode_dev): the 128 x 64 tiles of many grids of different shapes, each with a read pitch and a
// write pitch of its own, in ONE launch.
//
// A tile is coded from its own frame's bytes, so a tile of view i, staged from the same grid bytes at the
// same origin, runs exactly the code a lone pitched decode of that view runs: k_dec_pitched's fast path as it stands --
// pitched_buf, pitched_issue, stage_commit, the cone through the read pitch, dec_tile_fast / dec_tile_edge -- with W, H, the
// two 32-bit pitches, the two record counts and the two base pointers taken from the frame's 64-byte record (view_ctx) where
// that kernel takes them from its PitchedPlan and the frame stride.  In front of it stands the frame lists' "which frame am I":
// a binary search over the prefix array of the block's kind (hgi_views_plan.h, csrc/hgi_framelist.h).  Only the W bytes of a row
// are ever stored (interior chunks lie inside the row, store_rows_edge clips the ragged ones).  Buffer path only: the plan
// refuses a list with an entry whose offsets need 64 bits.
#define HGI_FUSED_NO_LAUNCHERS 1
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"                 // the uniform decode's host geometry and byte-checked staging:
#pragma clang diagnostic ignored "-Wunneeded-internal-declaration"   // this unit launches the buffer path only
#include "../csrc/hgi_fused_dec.hip"   // the decode direction's build settings and tile procedure, 128 x 64 tiles
#include "../csrc/hgi_fused_pitched.h"
#pragma clang diagnostic pop
#include "../companion/hgi_tile.h"
#include "hgi_views_tile.h"

namespace hgi {
namespace {

// One block (= one wave) per tile of the list.  SEEDED: 0 = the pyramid fits the tile (k = levels <= 5); 2 = the cone (k == 4,
// sd.up = levels - 4 levels above the tile, rebuilt from the frame's own base samples through its pitch).  The wave budget is
// k_dec_pitched's.
template <int INTERP, int SEEDED>
__global__ __launch_bounds__(NL) __attribute__((amdgpu_waves_per_eu(SEEDED == 2 ? HGI_DEC_WAVES_PER_EU - 2 : HGI_DEC_WAVES_PER_EU))) void k_dec_views(
    ViewArgs a, u32 k, Seeds sd)
{
    extern __shared__ __attribute__((aligned(16))) u8 smem[];
    const int nh = k >= 2 ? (int)k : 1;
    u8 *buf = smem - HCOL;
    const ViewTileCtx vc = view_ctx(a);
    if (vc.idle) return;
    const Tile tl = vc.tl;
    const PitchedPlan &p = vc.p;
    const u32 W = p.W, H = p.H;
    const u8 *fr = vc.fr;
    u8 *out = vc.out;
    const PitchAt at = {p.sp};
    SeedRegs seeds;
    ConeLane cone;
    u32 rb;
    TileCtx cur = {tl, pitched_buf(fr, out, p, tl, &rb)};
    Stage st;
    if (!vc.edge) {
        pitched_issue<false>(st, cur.b.rs, rb, p.sp32, W, tl, (int)k, nh);
        if (SEEDED == 2) cone = cone_issue<false>(fr, W, H, sd, tl, at);
        stage_commit<false>(buf, nullptr, st, nh);
        LDS_ORDER();
        pitched_issue_odd(st, cur.b.rs, rb, p.sp32);      // in flight while the coarse levels run (HGI_ODD_LATE)
        if (SEEDED == 2) seeds = cone_finish<INTERP, false, true>(cone, buf, nullptr, sd.up, nullptr);
        LDS_ORDER();
        if (SEEDED) dec_seed_commit(buf, seeds, k);
        dec_tile_fast<INTERP>(buf, cur, st.o, k, W, H);
        return;
    }
    if (SEEDED == 2) cone = cone_issue<false>(fr, W, H, sd, tl, at);
    pitched_issue<true, true>(st, cur.b.rs, rb, p.sp32, W, tl, (int)k, nh);
    stage_commit<false>(buf, nullptr, st, nh);
    LDS_ORDER();
    if (SEEDED == 2) seeds = cone_finish<INTERP, false, true>(cone, buf, nullptr, sd.up, nullptr);
    if (SEEDED) dec_seed_commit(buf, seeds, k);
    if (tl.X0 + TW <= W && !(H & 1u))
        dec_tile_edge<INTERP, 1>(buf, cur, st.o, k, W, H);
    else
        dec_tile_edge<INTERP, 2>(buf, cur, st.o, k, W, H);
}

}  // namespace

hipError_t launch_views_decode(const ViewArgs &a, uint32_t max_width, uint32_t k, uint32_t up, int interp, hipStream_t s)
{
    const TileLaunch t = views_tile_launch(a, k, up);
    if (!t.ok) return hipErrorInvalidValue;
    // resident tiles per CU: on the list's tile count and its widest frame
    const size_t lds = lds_for_waves((size_t)buf_bytes(t.nh), dec_resident_tiles((u64)a.nedge + a.nint, max_width, k, t.cone));
    return with_choices([&](auto I, auto SE) { return launch_tile_kernel<k_dec_views<I, SE>>(t.blocks, lds, s, a, k, t.sd); },
                        interp_choice(interp), OneOf<2, 0>{t.cone ? 2 : 0});
}

}  // namespace hgi
