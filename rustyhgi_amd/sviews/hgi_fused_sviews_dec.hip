// Scaled view-list decode (hgi_sviews_decode_dev): the 128 x 64 tiles of the 1 / 2^s images of many grids of different shapes,
// each read through a pitch of its own and written through a pitch of its own, in ONE launch.
//
// Two things the codec already has, one in front of the other:
//   * "which frame am I": the view lists' search (../views/hgi_views_tile.h, view_ctx) -- a binary search of the prefix array of
//     the block's kind by scalar loads, then the frame's 64-byte record in four scalar 16-byte loads;
//   * k_dec_scaled's fast path (../csrc/hgi_fused_scaled.hip) as it stands, call for call: scaled_issue_rows, the cone through
//     the view, stage_commit, scaled_issue_odd, the seed commits, dec_tile_fast / dec_tile_edge -- with the view (sw, sh, the
//     row pitch src_pitch << s, the span) and the output side (pitch, span) taken from the record where that kernel takes them
//     from its Scaled and the frame strides.  The record holds the view already (hgi_sviews_plan.h): the Scaled the staging
//     reads is filled in registers from it.
// The scaled unit is one anonymous-namespace unit and is included whole: k_dec_scaled, k_gather_view and its two launchers come
// along and stay unexported (DESIGN.md 4.21 says what that costs).  Buffer path only: the plan refuses a list with an entry whose
// offsets need 64 bits, and this unit has no byte-checked path, no device function and no store of its own.
#include "../csrc/hgi_fused_scaled.hip"   // the decode direction's unit without its launchers, the staging on a strided view
#include "../csrc/hgi_fused_pitched.h"
#include "../companion/hgi_tile.h"
#include "../views/hgi_views_tile.h"
#include "hgi_sviews_kernels.h"

namespace hgi {
namespace {

// One block (= one wave) per tile of the list's output images.  SEEDED: 0 = the remaining pyramid fits the tile (k <= 5); 2 = the
// cone (k == 4, sd.up levels above the tile).  SH: the interior tiles' loads (1, 2: wide loads for s = 1, 2; 0: byte loads).
// The wave budgets are k_dec_scaled's.
template <int INTERP, int SEEDED, int SH>
__global__ __launch_bounds__(NL) __attribute__((amdgpu_waves_per_eu(SH != 1 ? HGI_DEC_WAVES_PER_EU / 2 : SEEDED == 2 ? HGI_DEC_WAVES_PER_EU - 2 : HGI_DEC_WAVES_PER_EU))) void k_dec_sviews(
    ViewArgs a, u32 k, Seeds sd, u32 s)
{
    extern __shared__ __attribute__((aligned(16))) u8 smem[];
    const int nh = k >= 2 ? (int)k : 1;
    u8 *buf = smem - HCOL;
    const ViewTileCtx vc = view_ctx(a);
    if (vc.idle) return;
    const Tile tl = vc.tl;
    const PitchedPlan &p = vc.p;
    const u32 W = __builtin_amdgcn_readfirstlane(p.W), H = __builtin_amdgcn_readfirstlane(p.H);      // the view: sw x sh
    const u8 *fr = vc.fr;
    const bool edge = vc.edge;
    const ViewAt at = {(u64)__builtin_amdgcn_readfirstlane(p.sp32), s};
    Scaled sc = {};                  // what the staging reads of it: the view's width, its shift and its 32-bit row pitch
    sc.sw = W;
    sc.sh = H;
    sc.s = s;
    sc.rp32 = __builtin_amdgcn_readfirstlane(p.sp32);
    SeedRegs seeds;
    ConeLane cone;
    // 32-bit buffer offsets on both sides (the plan serves nothing else)
    Buf bo;   // the store side: the output image
    bo.rs = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(fr), 0, p.srec, 0x00020000);
    bo.rd = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(vc.out), 0, p.drec, 0x00020000);
    bo.W = p.dp32;
    bo.base = __builtin_amdgcn_readfirstlane(tl.Y0 * p.dp32 + tl.X0);
    const u32 vb = __builtin_amdgcn_readfirstlane(tl.Y0 * p.sp32 + (tl.X0 << s));
    Stage st;
    // (the wide-load kernels of s = 1 run at the tightest budgets: there the interior branch is laid out as the likely one, which
    // keeps every instantiation within k_dec_scaled's own register count; the branches themselves are that kernel's)
    if (SH == 1 ? __builtin_expect(!edge, 1) : !edge) {
        scaled_issue_rows<SH, false>(st, bo.rs, vb, sc, tl, (int)k, nh);
        if (SEEDED == 2) cone = cone_issue<false>(fr, W, H, sd, tl, at);
        stage_commit<false>(buf, nullptr, st, nh);
        LDS_ORDER();
        scaled_issue_odd<SH, false>(st, bo.rs, vb, sc, tl);      // in flight while the coarse levels run
    } else {
        if (SEEDED == 2) cone = cone_issue<false>(fr, W, H, sd, tl, at);
        scaled_issue_rows<0, true>(st, bo.rs, vb, sc, tl, (int)k, nh);
        scaled_issue_odd<0, true>(st, bo.rs, vb, sc, tl);
        stage_commit<false>(buf, nullptr, st, nh);
        LDS_ORDER();
    }
    if (SEEDED == 2) seeds = cone_finish<INTERP, false, true>(cone, buf, nullptr, sd.up, nullptr);
    LDS_ORDER();
    if (SEEDED) dec_seed_commit(buf, seeds, k);
    if (edge)
        dec_tile_edge<INTERP, 2>(buf, TileCtx{tl, bo}, st.o, k, W, H);
    else
        dec_tile_fast<INTERP>(buf, TileCtx{tl, bo}, st.o, k, W, H);
}

}  // namespace

hipError_t launch_sviews_decode(const ViewArgs &a, uint32_t max_width, uint32_t shift, uint32_t k, uint32_t up, int interp, hipStream_t s)
{
    const TileLaunch t = views_tile_launch(a, k, up);
    if (!t.ok || shift < 1 || shift > 31 || k > kSViewsMaxTileLevels) return hipErrorInvalidValue;
    // the decoder's layout; resident tiles per CU on the list's tile count and its widest image
    const size_t lds = lds_for_waves((size_t)buf_bytes(t.nh), dec_resident_tiles((u64)a.nedge + a.nint, max_width, k, t.cone));
    return with_choices([&](auto I, auto SE, auto SH) { return launch_tile_kernel<k_dec_sviews<I, SE, SH>>(t.blocks, lds, s, a, k, t.sd, shift); },
                        interp_choice(interp), OneOf<2, 0>{t.cone ? 2 : 0}, OneOf<1, 2, 0>{shift == 1 ? 1 : shift == 2 ? 2 : 0});
}

}  // namespace hgi
