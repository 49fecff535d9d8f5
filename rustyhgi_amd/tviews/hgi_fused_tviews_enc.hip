// Typed view-list encode (hgi_tviews_encode_dev): the 128 x 64 tiles of many frames of E-byte elements of different shapes,
// each read through a byte pitch of its own, converted (include/hgi_typed.h) and encoded into a grid written through a pitch of
// its own, in ONE launch.
//
// Two things the companions already have, one in front of the other:
//   * "which frame am I": the view lists' search (../views/hgi_views_tile.h, view_ctx) -- a binary search of the prefix array of
//     the block's kind by scalar loads, then the frame's 64-byte record in four scalar 16-byte loads;
//   * k_enc_typed's body (../typed/hgi_fused_typed_enc.hip) as it stands: typed_issue / typed_issue_odd / typed_convert_odd,
//     cone_issue_typed / cone_convert_typed, stage_commit, the table at LDS offset 0, cone_finish, enc_seed_commit,
//     enc_tile_fast / enc_tile_edge -- with W, H, the two descriptors and the two base offsets taken from the record where that
//     kernel takes them from its TypedPlan and the frame strides: the read side srec and rb = Y0 * sp32 + X0 * E in bytes
//     (hgi_tviews_plan.h), the written side drec and dp32 in pixels.
// The typed unit is one anonymous-namespace unit and is included whole: the staging, Cvt and kTypedWavesPerEu are what this unit
// uses; launch_encode_typed and the sixteen k_enc_typed kernels come along and stay unexported (DESIGN.md 4.19 says what that
// costs).  Buffer path only: the plan refuses a list with an entry whose offsets need 64 bits.
// Zero means pixel 0 (the typed unit's header): typed_issue predicates every load outside the image off and zeroes its pixels
// after conversion; the frame search in front changes nothing of that.  This unit has no store of its own: every store is the
// encoder tile's.
#include "../typed/hgi_fused_typed_enc.hip"   // the encode direction's unit, the pitched staging, the tile layer, the typed staging
#include "../views/hgi_views_tile.h"
#include "hgi_tviews_kernels.h"

namespace hgi {
namespace {

// One block (= one wave) per tile of the list.  SEEDED: 0 = the pyramid fits the tile (k = levels <= 5); 2 = the cone on the
// frame's own samples (k == 4, sd.up = levels - 4 levels above the tile).  E: bytes per element.  The wave budget is k_enc_typed's.
template <int INTERP, bool IDENT, int SEEDED, int E>
__global__ __launch_bounds__(NL) __attribute__((amdgpu_waves_per_eu(kTypedWavesPerEu))) void k_enc_tviews(
    ViewArgs a, u32 k, Lut256 lut, Seeds sd, Cvt cv)
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
    SeedRegs seeds;
    ConeLane cone;
    // 32-bit buffer offsets on both sides (the plan serves nothing else): bytes on the frame's side, pixels on the grid's
    TileCtx cur;
    cur.tl = tl;
    cur.b.rs = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(vc.fr), 0, p.srec, 0x00020000);
    cur.b.rd = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(vc.out), 0, p.drec, 0x00020000);
    cur.b.W = p.dp32;
    cur.b.base = __builtin_amdgcn_readfirstlane(tl.Y0 * p.dp32 + tl.X0);
    const u32 rb = __builtin_amdgcn_readfirstlane(tl.Y0 * p.sp32 + tl.X0 * E);
    Stage st;
    u32 lutv = 0;
    if (!vc.edge) {
        constexpr int NB = typed_batch(E);
        RawOdd<E> ro;
        typed_issue<E, false>(st, cur.b.rs, rb, p.sp32, W, H, tl, (int)k, nh, cv);
        typed_issue_odd<E>(ro, cur.b.rs, rb, p.sp32, 0);
        if (SEEDED == 2) cone = cone_issue_typed<E>(cur.b.rs, p.sp32, W, H, sd, tl);
        if (!IDENT) lutv = lut.w[HGI_LANE];
        stage_commit<true>(buf, rbuf, st, nh);
        if (!IDENT) reinterpret_cast<u32 *>(slut)[HGI_LANE] = lutv;
        LDS_ORDER();
        typed_convert_odd<E>(st, ro, cv, 0);
        if (NB < NFINE) {
            __builtin_amdgcn_sched_barrier(0);
            typed_issue_odd<E>(ro, cur.b.rs, rb, p.sp32, NB);
        }
        if (SEEDED == 2) {
            cone_convert_typed<E>(cone, cv);
            seeds = cone_finish<INTERP, true, IDENT>(cone, buf, rbuf, sd.up, slut);
        }
        enc_seed_commit<SEEDED>(buf, rbuf, seeds, k);
        if (NB < NFINE) typed_convert_odd<E>(st, ro, cv, NB);
        enc_tile_fast<INTERP, IDENT>(buf, rbuf, slut, cur, st.o, k, W, H);
        return;
    }
    if (SEEDED == 2) cone = cone_issue_typed<E>(cur.b.rs, p.sp32, W, H, sd, tl);
    typed_issue<E, true>(st, cur.b.rs, rb, p.sp32, W, H, tl, (int)k, nh, cv);
    if (!IDENT) lutv = lut.w[HGI_LANE];
    stage_commit<true>(buf, rbuf, st, nh);
    if (!IDENT) reinterpret_cast<u32 *>(slut)[HGI_LANE] = lutv;
    LDS_ORDER();
    if (SEEDED == 2) {
        cone_convert_typed<E>(cone, cv);
        seeds = cone_finish<INTERP, true, IDENT>(cone, buf, rbuf, sd.up, slut);
    }
    enc_seed_commit<SEEDED>(buf, rbuf, seeds, k);
    if (tl.X0 + TW <= W && !(H & 1u))
        enc_tile_edge<INTERP, IDENT, 1>(buf, rbuf, slut, cur, st.o, k, W, H);
    else
        enc_tile_edge<INTERP, IDENT, 2>(buf, rbuf, slut, cur, st.o, k, W, H);
}

}  // namespace

hipError_t launch_tviews_encode(const ViewArgs &a, uint32_t elem, bool bf16, float scale, float bias, uint32_t k, uint32_t up, int interp,
                                const Lut256 &lut, bool ident, hipStream_t s)
{
    const TileLaunch t = views_tile_launch(a, k, up);
    if (!t.ok || (elem != 2 && elem != 4) || (bf16 && elem != 2)) return hipErrorInvalidValue;
    const Cvt cv = {scale, bias, bf16 ? 1u : 0u};
    return with_choices(
        [&](auto I, auto ID, auto SE, auto EL) {
            return launch_tile_kernel<k_enc_tviews<I, ID != 0, SE, EL>>(t.blocks, enc_lds_bytes(t.nh), s, a, k, lut, t.sd, cv);
        },
        interp_choice(interp), OneOf<1, 0>{ident ? 1 : 0}, OneOf<2, 0>{t.cone ? 2 : 0}, OneOf<4, 2>{(int)elem});
}

}  // namespace hgi
