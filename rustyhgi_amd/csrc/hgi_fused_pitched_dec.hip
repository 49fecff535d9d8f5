// Pitched decode (hgi_decode_u8_pitched_dev): a batch of grids whose rows lie grid_pitch bytes apart, decoded into frames whose
// rows lie img_pitch bytes apart -- a crop of a larger grid plane into a window of a canvas, without a packing copy on
// either side.
//
// A tile is coded from its own frame's bytes, so the tile procedure of the fused decoder runs as it stands
// -- stage_commit, the cone, dec_tile_fast / dec_tile_edge -- with three launch constants where the uniform kernel has one:
// the read pitch (pitched_issue), the write pitch (Buf's W / base, as region and scaled decode address their output) and the
// image width (every test against the image).  The descriptors hold each frame's SPAN, (H - 1) * pitch + W: rows at and below
// H read 0 and are dropped when stored; only the W bytes of a row are ever stored (interior chunks lie inside the row,
// store_rows_edge clips the ragged ones), so the gap between rows keeps the caller's bytes.
// 128 x 64 tiles only; ragged tiles first, interior tiles row-major per frame in contiguous eighths (hgi_pitched.h).
#define HGI_FUSED_NO_LAUNCHERS 1
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"                 // the uniform decode's host geometry and byte-checked staging:
#pragma clang diagnostic ignored "-Wunneeded-internal-declaration"   // this unit has pitched forms of its own
#include "hgi_fused_dec.hip"   // the decode direction's build settings and tile procedure, 128 x 64 tiles
#include "hgi_fused_pitched.h"
#pragma clang diagnostic pop

namespace hgi {
namespace {

// One block (= one wave) per tile.  SEEDED: 0 = the pyramid fits the tile (k = levels <= 5); 2 = the cone (k == 4, sd.up levels
// above the tile, rebuilt from the frame's own base samples through the pitch, or from the stride-256 lattice planes).  The
// wave budget is k_dec_tiles'.
template <int INTERP, int SEEDED>
__global__ __launch_bounds__(NL) __attribute__((amdgpu_waves_per_eu(SEEDED == 2 ? HGI_DEC_WAVES_PER_EU - 2 : HGI_DEC_WAVES_PER_EU))) void k_dec_pitched(
    const u8 *__restrict__ src, u8 *__restrict__ dst, u32 k, Seeds sd, PitchedPlan p)
{
    extern __shared__ __attribute__((aligned(16))) u8 smem[];
    const int nh = k >= 2 ? (int)k : 1;
    u8 *buf = smem - HCOL;
    const u32 W = p.W, H = p.H;
    bool edge, idle;
    const Tile tl = pitched_block_tile(p, edge, idle);
    if (idle) return;
    const u8 *fr = src + (size_t)tl.frame * p.sstride;
    u8 *out = dst + (size_t)tl.frame * p.dstride;
    const PitchAt at = {p.sp};
    SeedRegs seeds;
    ConeLane cone;
    if (p.fast) {   // 32-bit buffer offsets on both sides
        u32 rb;
        TileCtx cur = {tl, pitched_buf(fr, out, p, tl, &rb)};
        Stage st;
        if (!edge) {
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
        return;
    }
    // frames whose byte offsets do not fit 32 bits (and the knobs build's HGI_FORCE_CHECKED): every access checked
    if (SEEDED == 2) cone = cone_issue<false>(fr, W, H, sd, tl, at);
    stage_pitched_generic(buf, fr, p.sp, W, H, tl, nh);
    LDS_ORDER();
    if (SEEDED == 2) seeds = cone_finish<INTERP, false, true>(cone, buf, nullptr, sd.up, nullptr);
    if (SEEDED) dec_seed_commit(buf, seeds, k);
    for (int s = 1 << (k - 1); s >= 2; s >>= 1) {
        dec_cells<INTERP, true>(buf, s, tl, W, H);
        dec_halo_cells<INTERP>(buf, s, tl, W, H);
        LDS_ORDER();
    }
    dec_fine_generic_pitched<INTERP>(buf, fr, out, tl, W, H, p.sp, p.dp);
}

}  // namespace

hipError_t launch_decode_pitched(const uint8_t *grid, uint8_t *img, const PitchedFrames &f, uint32_t k, int interp, const Seeds *seeds,
                                 hipStream_t s)
{
    if (k < 1 || k > (u32)MAXK || f.width == 0 || f.height == 0 || f.batch == 0) return hipErrorInvalidValue;
    const bool cone = seeds && seeds->up != 0;
    if (seeds && (!cone || k != 4 || seeds->up > (u32)kConeMaxUp)) return hipErrorInvalidValue;   // (no seed-plane route without a cone)
    const PitchedPlan p = pitched_plan(reinterpret_cast<uintptr_t>(grid), f, HGI_SWITCH(HGI_FORCE_CHECKED));
    if (!p.ok) return hipErrorInvalidValue;
    const Seeds sd = seeds ? *seeds : Seeds{nullptr, nullptr, 0, 0, 0, 0};
    const int nh = k >= 2 ? (int)k : 1;
    const size_t lds = lds_for_waves((size_t)buf_bytes(nh), dec_resident_tiles((u64)p.nf + p.nedge, f.width, k, seeds != nullptr));
    const dim3 blocks((u32)pitched_blocks(p));
    return with_choices([&](auto I, auto SE) { return launch_tile_kernel<k_dec_pitched<I, SE>>(blocks, lds, s, grid, img, k, sd, p); },
                        interp_choice(interp), OneOf<2, 0>{cone ? 2 : 0});
}

}  // namespace hgi
