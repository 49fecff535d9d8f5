// Recon view lists (hgi_rviews_encode_dev): the 128 x 64 tiles of many frames of different shapes, each read through a pitch of
// its own and written TWICE -- the grid and the image the decoder will make of it, each through a pitch of its own -- in ONE
// launch.
//
// Two things the companions already have, one in front of the other:
//   * "which frame am I": the view lists' search (../views/hgi_views_tile.h) -- list_role, a binary search of the prefix array
//     of the block's kind by scalar loads, the frame's 64-byte record in four scalar 16-byte loads, view_tile -- with the
//     frame index kept, because the third side stands in a parallel array: one more scalar 16-byte load.  The search is
//     rview_find (hgi_rviews_plan.h): list_find's result by a descent over fixed steps, unrolled, so that no cycle stands in
//     front of the tile body -- a cycle there, whatever it holds, costs the cone kernels three VGPRs;
//   * k_enc_recon's body (../recon/hgi_fused_recon_enc.hip) as it stands: the table at LDS offset 0, pitched_buf, tile_side on
//     the reconstruction, pitched_issue / stage_commit<true> / pitched_issue_odd, the cone on the frame's own samples
//     (cone_issue<true>, cone_finish), enc_seed_commit, enc_tile_fast_recon / enc_tile_edge_recon -- with W, H, the two 32-bit
//     pitches, the two descriptors' records and the frame's two pointers taken from the record where that kernel takes them
//     from its ReconPlan and the frame strides, and the third side's pitch, records and pointer from the parallel array.
// The recon unit is one anonymous-namespace unit and is included whole: enc_fine_recon and the two tile chains are what this
// unit uses; launch_encode_recon and the eight k_enc_recon kernels come along and stay unexported (DESIGN.md 4.22 says what
// that costs).  Buffer path only: the plan refuses a list with an entry whose offsets need 64 bits.
// This unit has no store of its own: every store is store_row_pair / store_rows_edge through enc_fine_recon.
#include "../recon/hgi_fused_recon_enc.hip"   // the encode direction's unit, the pitched staging, the tile layer, the recon tile chains
#include "../views/hgi_views_tile.h"
#include "hgi_rviews_kernels.h"

namespace hgi {
namespace {

// What a block starts from: view_ctx's context and the frame's third side.
struct RViewTileCtx {
    ViewTileCtx v;
    u8 *rout;
    ExtraSide x;
};

// view_ctx (../views/hgi_views_tile.h) with the frame index kept: the same role, the search's result by rview_find, the same record
// loads and tile, and one more
// scalar 16-byte load for the frame's third-side record.  Everything goes through the constant address space: every index is
// wave-uniform.
__device__ __forceinline__ RViewTileCtx rview_ctx(const RViewArgs &a)
{
#if HGI_ARGS_EARLY
    asm volatile("" ::"s"(a.v.frames), "s"(a.v.epre), "s"(a.v.ipre), "s"(a.recon), "s"(a.v.count), "s"(a.v.nedge), "s"(a.v.nint));
#endif
    RViewTileCtx c;
    ListBlock r = list_role(blockIdx.x, a.v.nedge, a.v.nint);
    c.v.edge = r.edge;
    c.v.idle = r.idle;
    if (r.idle) return c;
    view_cu32 *pre = (view_cu32 *)(r.edge ? a.v.epre : a.v.ipre);
    r.frame = rview_find(pre, a.v.count, r.t);      // list_find's result without a cycle in the kernel (hgi_rviews_plan.h)
    view_cv4 *rec = (view_cv4 *)a.v.frames + 4u * r.frame;
    view_cv4 *third = (view_cv4 *)a.recon + r.frame;
    const v4u words[4] = {rec[0], rec[1], rec[2], rec[3]};
    const v4u side = third[0];
    ViewFrame F;
    RViewSide S;
    __builtin_memcpy(&F, words, sizeof(F));
    __builtin_memcpy(&S, &side, sizeof(S));
    view_tile(r, F, pre[r.frame]);
    c.v.tl.frame = 0;      // (the records hold the frame's pointers: no frame stride, no seed planes)
    c.v.tl.X0 = __builtin_amdgcn_readfirstlane(r.tx * TW);
    c.v.tl.Y0 = __builtin_amdgcn_readfirstlane(r.ty * TH);
    c.v.fr = reinterpret_cast<const u8 *>(F.src);
    c.v.out = reinterpret_cast<u8 *>(F.dst);
    c.v.p = PitchedPlan{};
    c.v.p.W = F.width;
    c.v.p.H = F.height;
    c.v.p.fast = 1u;
    c.v.p.sp32 = F.sp32;
    c.v.p.dp32 = F.dp32;
    c.v.p.srec = F.srec;
    c.v.p.drec = F.drec;
    c.v.p.sp = F.sp32;
    c.v.p.dp = F.dp32;
    c.rout = reinterpret_cast<u8 *>(S.recon);
    c.x = ExtraSide{S.pitch32, S.rec, 0};
    return c;
}

// One block (= one wave) per tile of the list.  SEEDED: 0 the tile holds the pyramid (k = levels <= 5); 2 the cone on the
// frame's own samples (k == 4, sd.up = levels - 4 levels above the tile).  The wave budget is k_enc_recon's.
template <int INTERP, bool IDENT, int SEEDED>
__global__ __launch_bounds__(NL) __attribute__((amdgpu_waves_per_eu(IDENT ? HGI_ENC_WAVES_PER_EU - 1 : HGI_ENC_WAVES_PER_EU))) void k_enc_recon_views(
    RViewArgs a, u32 k, Lut256 lut, Seeds sd)
{
    extern __shared__ __attribute__((aligned(16))) u8 smem[];
    const int nh = k >= 2 ? (int)k : 1;
    // the table at LDS offset 0 (lut_at(); launch_tile_kernel checks on the host that there is no static LDS)
    u8 *slut = smem;
    u8 *buf = smem + 256 - HCOL;
    u8 *rbuf = smem + 256 + buf_bytes(nh) - RCOL;
    const RViewTileCtx rc = rview_ctx(a);
    if (rc.v.idle) return;
    const Tile tl = rc.v.tl;
    const PitchedPlan &p = rc.v.p;
    const u32 W = p.W, H = p.H;
    const u8 *fr = rc.v.fr;
    u8 *out = rc.v.out;
    u8 *rout = rc.rout;
    const PitchAt at = {p.sp};
    u32 lutv = 0;
    SeedRegs seeds;
    ConeLane cone;
    // 32-bit buffer offsets on all three sides (the plan serves nothing else)
    u32 rb;
    TileCtx cur = {tl, pitched_buf(fr, out, p, tl, &rb)};
    const TileSide ro = tile_side(rc.x, rout, tl, 1);
    Stage st;
    if (!rc.v.edge) {
        pitched_issue<false>(st, cur.b.rs, rb, p.sp32, W, tl, (int)k, nh);
        if (SEEDED == 2) cone = cone_issue<true>(fr, W, H, sd, tl, at);
        if (!IDENT) lutv = lut.w[HGI_LANE];
        stage_commit<true>(buf, rbuf, st, nh);
        if (!IDENT) reinterpret_cast<u32 *>(slut)[HGI_LANE] = lutv;
        LDS_ORDER();
        pitched_issue_odd(st, cur.b.rs, rb, p.sp32);
        if (SEEDED == 2) seeds = cone_finish<INTERP, true, IDENT>(cone, buf, rbuf, sd.up, slut);
        enc_seed_commit<SEEDED>(buf, rbuf, seeds, k);
        enc_tile_fast_recon<INTERP, IDENT>(buf, rbuf, slut, cur, ro, st.o, k, W, H);
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
        enc_tile_edge_recon<INTERP, IDENT, 1>(buf, rbuf, slut, cur, ro, st.o, k, W, H);
    else
        enc_tile_edge_recon<INTERP, IDENT, 2>(buf, rbuf, slut, cur, ro, st.o, k, W, H);
}

}  // namespace

hipError_t launch_rviews_encode(const RViewArgs &a, uint32_t k, uint32_t up, int interp, const Lut256 &lut, bool ident, hipStream_t s)
{
    const TileLaunch t = views_tile_launch(a.v, k, up);
    if (!t.ok) return hipErrorInvalidValue;
    return with_choices(
        [&](auto I, auto ID, auto SE) {
            return launch_tile_kernel<k_enc_recon_views<I, ID != 0, SE>>(t.blocks, enc_lds_bytes(t.nh), s, a, k, lut, t.sd);
        },
        interp_choice(interp), OneOf<1, 0>{ident ? 1 : 0}, OneOf<2, 0>{t.cone ? 2 : 0});
}

}  // namespace hgi
