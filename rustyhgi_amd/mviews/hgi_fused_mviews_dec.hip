// Mapped view-list decode (hgi_mviews_decode_dev): the 128 x 64 tiles of many grids of different shapes, each read through a
// pitch of its own and written as E-byte elements, out[p] = table[decoded[p]], through a byte pitch of its own, in ONE launch.
//
// Two things the companions already have, one in front of the other:
//   * "which frame am I": the view lists' search (../views/hgi_views_tile.h, view_ctx) -- a binary search of the prefix array of
//     the block's kind by scalar loads, then the frame's 64-byte record in four scalar 16-byte loads;
//   * k_dec_map's body (../map/hgi_fused_map_dec.hip) as it stands: pitched_issue, the lane's 4 * E bytes of the table issued
//     with the staging loads, stage_commit, the cone through the read pitch, the seed commits, dec_tile_map -- with W, H, the
//     read pitch and record count and the two base pointers taken from the record where that kernel takes them from its MapPlan
//     and the frame strides, and the written side a TileSide of the record's dst, dp32 (the byte pitch) and drec (the span in
//     bytes, hgi_mviews_plan.h).
// The mapped unit is one anonymous-namespace unit and is included whole: dec_tile_map, TabLane, map_waves_per_eu and
// kMapStageBytes are what this unit uses; launch_decode_map and the eight k_dec_map kernels come along and stay unexported
// (DESIGN.md 4.18 says what that costs).  Buffer path only: the plan refuses a list with an entry whose offsets need 64 bits.
// Every store wider than 64 bits goes through store_map_rows.
#include "../map/hgi_fused_map_dec.hip"   // the decode direction's unit, the pitched staging, the tile layer, the mapped finest pass
#include "../views/hgi_views_tile.h"
#include "hgi_mviews_kernels.h"

namespace hgi {
namespace {

// One block (= one wave) per tile of the list.  SEEDED: 0 = the pyramid fits the tile (k = levels <= 5); 2 = the cone (k == 4,
// sd.up = levels - 4 levels above the tile).  E: bytes per output element.  The wave budgets are k_dec_map's.
template <int INTERP, int SEEDED, int E>
__global__ __launch_bounds__(NL) __attribute__((amdgpu_waves_per_eu(map_waves_per_eu(SEEDED, E)))) void k_dec_mviews(
    ViewArgs a, const u8 *__restrict__ tabg, u32 k, Seeds sd)
{
    extern __shared__ __attribute__((aligned(16))) u8 smem[];
    const int nh = k >= 2 ? (int)k : 1;
    u8 *buf = smem - HCOL;
    u8 *tab = smem + buf_bytes(nh);      // behind the decoder's layout (launch_tile_kernel checks that there is no static LDS)
    const ViewTileCtx vc = view_ctx(a);
    if (vc.idle) return;
    const Tile tl = vc.tl;
    const PitchedPlan &p = vc.p;
    const u32 W = p.W, H = p.H;
    const u8 *fr = vc.fr;
    const PitchAt at = {p.sp};
    // 32-bit buffer offsets on both sides (the plan serves nothing else)
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(fr), 0, p.srec, 0x00020000);
    const u32 rb = __builtin_amdgcn_readfirstlane(tl.Y0 * p.sp32 + tl.X0);
    const ExtraSide x = {p.dp32, p.drec, 0};
    const TileSide mo = tile_side(x, vc.out, tl, E);
    SeedRegs seeds;
    ConeLane cone;
    Stage st;
    TabLane<E> tv;
    if (!vc.edge) {
        pitched_issue<false>(st, rs, rb, p.sp32, W, tl, (int)k, nh);
        __builtin_memcpy(&tv, tabg + 4 * E * HGI_LANE, 4 * E);
        if (SEEDED == 2) cone = cone_issue<false>(fr, W, H, sd, tl, at);
        stage_commit<false>(buf, nullptr, st, nh);
        *reinterpret_cast<TabLane<E> *>(tab + 4 * E * HGI_LANE) = tv;
        LDS_ORDER();
        pitched_issue_odd(st, rs, rb, p.sp32);      // in flight while the coarse levels run
        if (SEEDED == 2) seeds = cone_finish<INTERP, false, true>(cone, buf, nullptr, sd.up, nullptr);
        LDS_ORDER();
        if (SEEDED) dec_seed_commit(buf, seeds, k);
        dec_tile_map<INTERP, E, 0>(buf, tab, tl, mo, st.o, k, W, H);
        return;
    }
    if (SEEDED == 2) cone = cone_issue<false>(fr, W, H, sd, tl, at);
    pitched_issue<true, true>(st, rs, rb, p.sp32, W, tl, (int)k, nh);
    __builtin_memcpy(&tv, tabg + 4 * E * HGI_LANE, 4 * E);
    stage_commit<false>(buf, nullptr, st, nh);
    *reinterpret_cast<TabLane<E> *>(tab + 4 * E * HGI_LANE) = tv;
    LDS_ORDER();
    if (SEEDED == 2) seeds = cone_finish<INTERP, false, true>(cone, buf, nullptr, sd.up, nullptr);
    if (SEEDED) dec_seed_commit(buf, seeds, k);
    if (tl.X0 + TW <= W && !(H & 1u))
        dec_tile_map<INTERP, E, 1>(buf, tab, tl, mo, st.o, k, W, H);
    else
        dec_tile_map<INTERP, E, 2>(buf, tab, tl, mo, st.o, k, W, H);
}

}  // namespace

hipError_t launch_mviews_decode(const ViewArgs &a, uint32_t max_width, const void *table, uint32_t elem, uint32_t k, uint32_t up, int interp,
                                hipStream_t s)
{
    const TileLaunch t = views_tile_launch(a, k, up);
    if (!t.ok || (elem != 2 && elem != 4)) return hipErrorInvalidValue;
    // the decoder's layout, the table and the staging rows behind it; resident tiles per CU on the list's tile count and its
    // widest frame
    const size_t lds = lds_for_waves((size_t)buf_bytes(t.nh) + 256 * (size_t)elem + kMapStageBytes,
                                     dec_resident_tiles((u64)a.nedge + a.nint, max_width, k, t.cone));
    const u8 *tab = static_cast<const u8 *>(table);
    return with_choices([&](auto I, auto SE, auto EL) { return launch_tile_kernel<k_dec_mviews<I, SE, EL>>(t.blocks, lds, s, a, tab, k, t.sd); },
                        interp_choice(interp), OneOf<2, 0>{t.cone ? 2 : 0}, OneOf<4, 2>{(int)elem});
}

}  // namespace hgi
