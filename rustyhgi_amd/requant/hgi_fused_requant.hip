// Requantize (hgi_requant_dev): a grid re-coded with another quantizer table, grid in and grid out, in one launch.
// Each tile runs BOTH level chains of the codec on the same LDS planes:
//   1. the source GRID is staged the way the decoder stages it (pitched_issue, stage_commit<false>), into the encoder's LDS
//      layout -- the table at offset 0, `buf`, `rbuf` -- with the table's load issued behind the staging loads;
//   2. the decoder's chain runs in place in `buf` as it stands (dec_cells / dec_halo_cells per coarse level, dec_level2_fast);
//      after it every even/even lattice point of body and halo holds the decoded pixel;
//   3. `rbuf` is made from `buf` (lattice_fast: what stage_commit<true> writes from registers) -- the finest pass changes no
//      even/even byte, so the copy can run in front of it;
//   4. dec_fine_keep, the one new pass: dec_fine_fast's arithmetic without its stores -- the decoded even rows go back to their
//      `buf` rows, the decoded odd rows stay in the registers the staging loads put them in;
//   5. the encoder's chain runs as it stands (enc_tile_fast / enc_tile_edge) on those planes and registers -- they now hold what
//      staging the DECODED image would have left -- and stores the new grid through the destination's descriptor and pitch.
// Levels 6 ... 8 (SEEDED == 2): one cone_issue on the source grid; cone_finish in decode mode gives the decoded values of the 54
// cone points and the tile's seeds; after the decoder's chain a second cone_finish in encode mode, fed with those decoded values
// instead of a load, gives the seeds' reconstruction and residual under the new table.
// 2 B/px of traffic instead of the 4 B/px of a decode launch and an encode launch.  This is the 64-row build of the encoder,
// buffer path only: hgi_requant.hip refuses the calls whose offsets need 64 bits, and the identity table (under it the result is
// the source: no kernel is instantiated for it).
#define HGI_FUSED_NO_LAUNCHERS 1
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"
#pragma clang diagnostic ignored "-Wunneeded-internal-declaration"
#include "../csrc/hgi_fused_enc.hip"   // the encode direction's build settings and tile procedure, 128 x 64 tiles
#include "../csrc/hgi_fused_pitched.h"
#pragma clang diagnostic pop
#include "../companion/hgi_tile.h"
#include "hgi_requant_kernels.h"

namespace hgi {
namespace {

// The half-resolution plane from the even-row plane, out of LDS: the even bytes of every staged row (body and halo rows) and the
// transposed halo columns -- stage_commit<true>'s lattice writes, lattice_from_buf without its divisions.
__device__ __forceinline__ void lattice_fast(const u8 *buf, u8 *rbuf, int nh)
{
    const int lane = HGI_LANE, c = lane & (CH - 1), r = lane >> LCH;
#pragma unroll
    for (int j = 0; j < TH / 16; ++j)
        *reinterpret_cast<v2u *>(rbuf + (r + 8 * j) * S2 + 8 * c) = even_bytes(*reinterpret_cast<const v4u *>(buf + (r + 8 * j) * S + 16 * c));
    if (lane < nh * CH)
        *reinterpret_cast<v2u *>(rbuf + (TH / 2 + r) * S2 + 8 * c) = even_bytes(*reinterpret_cast<const v4u *>(buf + (TH / 2 + r) * S + 16 * c));
    if (lane < TH / 2 + nh) {
        const u8 *h = buf + HCOL + lane;
        u8 *h2 = rbuf + RCOL + lane;
        u32 v[HR];
#pragma unroll
        for (int i = 0; i < HR; ++i) v[i] = h[i * HP];
#pragma unroll
        for (int i = 0; i < HR; ++i) h2[i * HP2] = (u8)v[i];
    }
}

// dec_fine_fast without the stores: same lane map, same loads, same arithmetic.  The decoded even row of a task goes back to
// its `buf` row -- only its odd columns change, so the lanes that read the row as their lower lattice row (even columns) see the
// same bytes before and after -- and the decoded odd row replaces the residuals in odd[it]: the encoder's finest pass uses the
// same lane map and takes both unchanged.
// EDGE (as dec_fine_fast): everything outside the `rows` x `cols` part of the tile inside the image was staged as zero and
// stays zero.  EDGE == 1 (full width inside, even height): a row pair below the image has zero residuals and zero corners, so
// its prediction is zero and it stays zero by arithmetic.  EDGE == 2: columns right of the image are masked, an odd row below
// the image is cleared, an even row below it is not written.
template <int INTERP, int EDGE = 0>
__device__ __forceinline__ void dec_fine_keep(u8 *buf, v4u (&odd)[NFINE], int rows = TH, int cols = TW)
{
    const int lane = HGI_LANE;
    const int rp0 = fine_pair0();
    const bool last = (lane & (CH - 1)) == CH - 1;
    u8 *r0 = buf + rp0 * S + 16 * (lane & (CH - 1));
    const u8 *h0 = buf + HCOL + rp0;
    const v4u cm = EDGE == 2 ? chunk_mask(cols - 16 * (lane & (CH - 1))) : v4u{~0u, ~0u, ~0u, ~0u};
#pragma unroll
    for (int it = 0; it < NFINE; ++it, r0 += (NL / CH) * S, h0 += NL / CH) {
        v4u E = *reinterpret_cast<const v4u *>(r0);
        v4u O = odd[it];
        v4u F = *reinterpret_cast<const v4u *>(r0 + S);
        // ninth corner of each lattice row: first byte of the next chunk = lane + 1, or the halo column
        u32 e16 = from_next_lane(E.x), f16 = from_next_lane(F.x);
        const u32 he = h0[0], hf = h0[1];
        e16 = last ? he : e16;
        f16 = last ? hf : f16;
        v4u r0v, r1v;
        dec_fine_rows<INTERP>(E, F, e16, f16, O, r0v, r1v);
        if (EDGE == 2) {
            const int y = 2 * (rp0 + it * (NL / CH));
            r0v &= cm;
            r1v &= cm;
            if (y + 1 >= rows) r1v = v4u{0, 0, 0, 0};
            if (y < rows) *reinterpret_cast<v4u *>(r0) = r0v;
        } else {
            *reinterpret_cast<v4u *>(r0) = r0v;
        }
        odd[it] = r1v;
    }
}

// The cone's second walk, in encode mode.  Its inputs are the DECODED values of the cone points, which the first walk left in
// the reconstruction array (one byte per lane; a four-level tile touches the array's halo-column slots of `buf` at staging
// only, so the decoder's chain has not disturbed it) -- read here into the lane before the walk rewrites the array level by
// level.  The seeds' inputs are read by the walk itself from the stride-16 points of `buf`, which dec_seed_commit filled with
// decoded values.  The residual array lives in the same slots of `rbuf` and is written by this walk alone (lattice_fast copied
// `buf`'s slots there; the walk writes every entry before it reads it).
template <int INTERP>
__device__ __forceinline__ SeedRegs cone_recode(const ConeLane &c, u8 *buf, u8 *rbuf, u32 up, const u8 *slut)
{
    ConeLane e = c;
    e.v = e.vq = cone_rec_array(buf)[HGI_LANE];      // base samples: the residual is the sample
    e.framed1 = false;                               // the value is in hand; the staged frame holds the same at such a point
    LDS_ORDER();
    return cone_finish<INTERP, true, false>(e, buf, rbuf, up, slut);
}

// SEEDED: 0 the tile holds the pyramid, 2 the cone on the source grid (k == 4).  The wave budget is k_enc_pitched's.
template <int INTERP, int SEEDED>
__global__ __launch_bounds__(NL) __attribute__((amdgpu_waves_per_eu(HGI_ENC_WAVES_PER_EU))) void k_requant(
    const u8 *__restrict__ src, u8 *__restrict__ dst, u32 k, Lut256 lut, Seeds sd, PitchedPlan p)
{
    extern __shared__ __attribute__((aligned(16))) u8 smem[];
    const int nh = k >= 2 ? (int)k : 1;
    // the encoder's layout: the table at LDS offset 0 (lut_at(); launch_requant checks on the host that there is no static LDS)
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
    // 32-bit buffer offsets on both sides (the host launches nothing else)
    u32 rb;
    TileCtx cur = {tl, pitched_buf(fr, out, p, tl, &rb)};
    Stage st;
    if (!edge) {
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

hipError_t launch_requant(const uint8_t *src, uint8_t *dst, const PitchedPlan &p, uint32_t k, uint32_t up, int interp,
                          const Lut256 &lut, hipStream_t s)
{
    const TileLaunch t = tile_launch(p, k, up);
    if (!t.ok) return hipErrorInvalidValue;
    return with_choices(
        [&](auto I, auto SE) { return launch_tile_kernel<k_requant<I, SE>>(t.blocks, enc_lds_bytes(t.nh), s, src, dst, k, lut, t.sd, p); },
        interp_choice(interp), OneOf<2, 0>{t.cone ? 2 : 0});
}

}  // namespace hgi
