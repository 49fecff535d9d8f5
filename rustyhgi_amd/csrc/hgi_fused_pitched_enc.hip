// Pitched encode (hgi_encode_u8_pitched_dev): a batch of images whose rows lie img_pitch bytes apart -- a crop of a larger
// device image, a plane with padded rows -- encoded into grids whose rows lie grid_pitch bytes apart.  The decode unit
// (hgi_fused_pitched_dec.hip) says how the three launch constants -- read pitch, write pitch, image width -- enter the tile
// procedure; each tile then runs k_enc_tiles' procedure as it stands: the table in LDS, the cone, enc_tile_fast /
// enc_tile_edge.  This is the 64-row build of the encoder; the uniform plain encode runs 32-row tiles on most calls
// (hgi_capi.hip use_tile_rows), and a 32-row pitched encoder is not built.
#define HGI_FUSED_NO_LAUNCHERS 1
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"
#pragma clang diagnostic ignored "-Wunneeded-internal-declaration"
#include "hgi_fused_enc.hip"   // the encode direction's build settings and tile procedure, 128 x 64 tiles
#include "hgi_fused_pitched.h"
#pragma clang diagnostic pop

namespace hgi {
namespace {

// SEEDED: as in k_dec_pitched (with seed planes the lattice's residuals come with them: sd.q).  The wave budget is k_enc_tiles'.
template <int INTERP, bool IDENT, int SEEDED>
__global__ __launch_bounds__(NL) __attribute__((amdgpu_waves_per_eu(IDENT ? HGI_ENC_WAVES_PER_EU - 1 : HGI_ENC_WAVES_PER_EU))) void k_enc_pitched(
    const u8 *__restrict__ src, u8 *__restrict__ dst, u32 k, Lut256 lut, Seeds sd, PitchedPlan p)
{
    extern __shared__ __attribute__((aligned(16))) u8 smem[];
    const int nh = k >= 2 ? (int)k : 1;
    // the table at LDS offset 0 (lut_at(); launch_encode_pitched checks on the host that there is no static LDS)
    u8 *slut = smem;
    u8 *buf = smem + 256 - HCOL;
    u8 *rbuf = smem + 256 + buf_bytes(nh) - RCOL;
    const u32 W = p.W, H = p.H;
    bool edge, idle;
    const Tile tl = pitched_block_tile(p, edge, idle);
    if (idle) return;
    const u8 *fr = src + (size_t)tl.frame * p.sstride;
    u8 *out = dst + (size_t)tl.frame * p.dstride;
    const PitchAt at = {p.sp};
    u32 lutv = 0;
    SeedRegs seeds;
    ConeLane cone;
    if (p.fast) {   // 32-bit buffer offsets on both sides
        u32 rb;
        TileCtx cur = {tl, pitched_buf(fr, out, p, tl, &rb)};
        Stage st;
        if (!edge) {
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
        return;
    }
    // frames whose byte offsets do not fit 32 bits (and the knobs build's HGI_FORCE_CHECKED): every access checked
    if (SEEDED == 2) cone = cone_issue<true>(fr, W, H, sd, tl, at);
    if (!IDENT) reinterpret_cast<u32 *>(slut)[HGI_LANE] = lut.w[HGI_LANE];
    stage_pitched_generic(buf, fr, p.sp, W, H, tl, nh);
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
    enc_fine_generic_pitched<INTERP, IDENT>(buf, rbuf, slut, fr, out, tl, W, H, p.sp, p.dp);
}

}  // namespace

hipError_t launch_encode_pitched(const uint8_t *img, uint8_t *grid, const PitchedFrames &f, uint32_t k, int interp, const Lut256 &lut,
                                 bool ident, const Seeds *seeds, hipStream_t s)
{
    if (k < 1 || k > (u32)MAXK || f.width == 0 || f.height == 0 || f.batch == 0) return hipErrorInvalidValue;
    const bool cone = seeds && seeds->up != 0;
    if (seeds && (!cone || k != 4 || seeds->up > (u32)kConeMaxUp || !seeds->rec != !seeds->q)) return hipErrorInvalidValue;
    const PitchedPlan p = pitched_plan(reinterpret_cast<uintptr_t>(img), f, HGI_SWITCH(HGI_FORCE_CHECKED));
    if (!p.ok) return hipErrorInvalidValue;
    const Seeds sd = seeds ? *seeds : Seeds{nullptr, nullptr, 0, 0, 0, 0};
    const int nh = k >= 2 ? (int)k : 1;
    const size_t lds = lds_for_waves(enc_lds_bytes(nh), HGI_KNOB(HGI_ENC_WAVES, 0));
    const dim3 blocks((u32)pitched_blocks(p));
    return with_choices(
        [&](auto I, auto ID, auto SE) { return launch_tile_kernel<k_enc_pitched<I, ID != 0, SE>>(blocks, lds, s, img, grid, k, lut, sd, p); },
        interp_choice(interp), OneOf<1, 0>{ident ? 1 : 0}, OneOf<2, 0>{cone ? 2 : 0});
}

}  // namespace hgi
