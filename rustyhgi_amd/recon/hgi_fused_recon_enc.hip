// Encode with reconstruction (hgi_recon_encode_u8_dev): the grid AND the image the decoder will make of it, in one launch.
// Each tile runs k_enc_pitched's procedure (csrc/hgi_fused_pitched_enc.hip) as it stands -- the table in LDS, the cone, the
// coarse-level chain, level 2 -- and a finest pass of its own, enc_fine_recon, which forms the two reconstruction rows of a
// task from what enc_fine_fast already holds when it stores the grid, and stores them through a second write descriptor:
//   row y     even columns: the even/even lattice's reconstruction, the corners the pass loaded from rbuf for its predictor;
//             odd columns:  coded residual + prediction;
//   row y + 1 coded residual + prediction throughout.
// That is what the decoder's finest pass computes from the grid (dec_fine_fast), so the second output is bit for bit
// hgi_decode_u8_dev of the first.  3 B/px of traffic instead of the 4 B/px of an encode launch and a decode launch.
// This is the 64-row build of the encoder, buffer path only: hgi_recon.hip refuses the calls whose offsets need 64 bits.
#define HGI_FUSED_NO_LAUNCHERS 1
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"
#pragma clang diagnostic ignored "-Wunneeded-internal-declaration"
#include "../csrc/hgi_fused_enc.hip"   // the encode direction's build settings and tile procedure, 128 x 64 tiles
#include "../csrc/hgi_fused_pitched.h"
#pragma clang diagnostic pop
#include "../companion/hgi_tile.h"
#include "hgi_recon_kernels.h"

namespace hgi {
namespace {

// enc_fine_fast with the reconstruction: same lane map, same loads, same grid stores; per task eight packed adds, eight byte
// permutes and one more row pair stored.  A task's grid rows are stored before its reconstruction rows are formed, so the
// two row pairs are not live together for longer than the adds take.
template <int INTERP, bool IDENT, int EDGE = 0>
__device__ __forceinline__ void enc_fine_recon(const u8 *buf, const u8 *rbuf, const u8 *slut, const Buf &b, const TileSide &ro,
                                               const v4u (&odd)[NFINE], int rows = TH, int cols = TW)
{
    const int lane = HGI_LANE;
    const int rp0 = fine_pair0();
    const bool last = (lane & (CH - 1)) == CH - 1;
    const u8 *r0 = buf + rp0 * S + 16 * (lane & (CH - 1));
    const u8 *c0 = rbuf + rp0 * S2 + 8 * (lane & (CH - 1));
    const u8 *h0 = rbuf + RCOL + rp0;
    u32 voff = b.base + 2 * rp0 * b.W + 16 * (lane & (CH - 1));
    u32 roff = ro.base + 2 * rp0 * ro.pitch + 16 * (lane & (CH - 1));
    const u32 Ws = __builtin_amdgcn_readfirstlane(b.W), Wr = __builtin_amdgcn_readfirstlane(ro.pitch);
    constexpr int NIT = NFINE, PAIR = NFINE >= 2 ? 2 : 1;   // row-pair groups per LDS dependency chain (enc_fine_fast's batch)
    static_assert(NIT % PAIR == 0, "fine level iterations come in pairs");
#pragma unroll
    for (int it = 0; it < NIT; it += PAIR) {
        v4u E_[PAIR], O_[PAIR];
        uint2 c_[PAIR], f_[PAIR];
        u32 hc_[PAIR], hf_[PAIR];
#pragma unroll
        for (int j = 0; j < PAIR; ++j) {
            const u8 *r = r0 + j * (NL / CH) * S, *c = c0 + j * (NL / CH) * S2, *h = h0 + j * (NL / CH);
            E_[j] = *reinterpret_cast<const v4u *>(r);
            O_[j] = odd[it + j];
            c_[j] = *reinterpret_cast<const uint2 *>(c);
            f_[j] = *reinterpret_cast<const uint2 *>(c + S2);
            hc_[j] = h[0];
            hf_[j] = h[1];
        }
#pragma unroll
        for (int j = 0; j < PAIR; ++j) {
            const v4u E = E_[j], O = O_[j];
            const uint2 c = c_[j], fl = f_[j];
            // ninth corner of each lattice row: lane + 1, or the transposed halo column
            u32 c8 = from_next_lane(c.x), f8 = from_next_lane(fl.x);
            c8 = last ? hc_[j] : c8;
            f8 = last ? hf_[j] : f8;
            u32 P0, P1;
            pred8<INTERP>(c, c8, fl, f8, P0, P1);
            u32 e0 = E.x, e1 = E.y, e2 = E.z, e3 = E.w, g0 = O.x, g1 = O.y, g2 = O.z, g3 = O.w;
            const u32 oddb = 0xFF00FF00u;
            const u32 pp0 = __builtin_amdgcn_perm(P0, P0, 0x01010000u), pp1 = __builtin_amdgcn_perm(P0, P0, 0x03030202u);
            const u32 pp2 = __builtin_amdgcn_perm(P1, P1, 0x01010000u), pp3 = __builtin_amdgcn_perm(P1, P1, 0x03030202u);
            if (IDENT) {
                e0 = sub4(e0, pp0 & oddb); e1 = sub4(e1, pp1 & oddb); e2 = sub4(e2, pp2 & oddb); e3 = sub4(e3, pp3 & oddb);
                g0 = sub4(g0, pp0); g1 = sub4(g1, pp1); g2 = sub4(g2, pp2); g3 = sub4(g3, pp3);
            } else {
                const u32 N0 = ~P0, N1 = ~P1;
                // row y: only the odd columns are new (cell j of the lane = byte j of P0, or byte j-4 of P1)
                Q_PIX4(slut, P0, N0, e0, 1, 0, e0, 3, 1, e1, 1, 2, e1, 3, 3);
                Q_PIX4(slut, P1, N1, e2, 1, 0, e2, 3, 1, e3, 1, 2, e3, 3, 3);
                // row y+1: every column
                Q_PIX4(slut, P0, N0, g0, 0, 0, g0, 1, 0, g0, 2, 1, g0, 3, 1);
                Q_PIX4(slut, P0, N0, g1, 0, 2, g1, 1, 2, g1, 2, 3, g1, 3, 3);
                Q_PIX4(slut, P1, N1, g2, 0, 0, g2, 1, 0, g2, 2, 1, g2, 3, 1);
                Q_PIX4(slut, P1, N1, g3, 0, 2, g3, 1, 2, g3, 2, 3, g3, 3, 3);
            }
            const v4u o0 = {e0, e1, e2, e3}, o1 = {g0, g1, g2, g3};
            const u32 vo = voff + j * 2 * (NL / CH) * Ws, vr = roff + j * 2 * (NL / CH) * Wr;
            const int y = 2 * (rp0 + (it + j) * (NL / CH)), nvalid = cols - 16 * (lane & (CH - 1));
            if (EDGE == 2)
                store_rows_edge(o0, o1, b.rd, vo, Ws, nvalid, y < rows, y + 1 < rows);
            else
                store_row_pair(o0, o1, b.rd, vo, Ws);
            // the reconstruction: lattice bytes (c byte i = column 2 i) interleaved with the odd columns of row y ...
            v4u q0, q1;
            if (IDENT) {     // ... which for the identity table are the image's own bytes
                q0 = v4u{__builtin_amdgcn_perm(E.x, c.x, 0x07010500u), __builtin_amdgcn_perm(E.y, c.x, 0x07030502u),
                         __builtin_amdgcn_perm(E.z, c.y, 0x07010500u), __builtin_amdgcn_perm(E.w, c.y, 0x07030502u)};
                q1 = O;
            } else {
                q0 = v4u{add4(__builtin_amdgcn_perm(e0, c.x, 0x07010500u), pp0 & oddb), add4(__builtin_amdgcn_perm(e1, c.x, 0x07030502u), pp1 & oddb),
                         add4(__builtin_amdgcn_perm(e2, c.y, 0x07010500u), pp2 & oddb), add4(__builtin_amdgcn_perm(e3, c.y, 0x07030502u), pp3 & oddb)};
                q1 = v4u{add4(g0, pp0), add4(g1, pp1), add4(g2, pp2), add4(g3, pp3)};
            }
            if (EDGE == 2)
                store_rows_edge(q0, q1, ro.r, vr, Wr, nvalid, y < rows, y + 1 < rows);
            else
                store_row_pair(q0, q1, ro.r, vr, Wr);
        }
        r0 += PAIR * (NL / CH) * S;
        c0 += PAIR * (NL / CH) * S2;
        h0 += PAIR * (NL / CH);
        voff += PAIR * 2 * (NL / CH) * Ws;
        roff += PAIR * 2 * (NL / CH) * Wr;
    }
}

// enc_tile_edge's chain with the new last link
template <int INTERP, bool IDENT, int EDGE>
__device__ __forceinline__ void enc_tile_edge_recon(u8 *buf, u8 *rbuf, const u8 *slut, const TileCtx &cur, const TileSide &ro,
                                                    const v4u (&odd)[NFINE], u32 k, u32 W, u32 H)
{
#define HGI_ENC_EDGE_COARSE(SUB)                                                   \
    if (k > HGI_LOG2(SUB)) {                                                       \
        enc_cells<INTERP, IDENT, true>(buf, rbuf, slut, SUB, cur.tl, W, H);        \
        enc_halo_pass<INTERP, IDENT>(buf, rbuf, slut, SUB, cur.tl, W, H);          \
        LDS_ORDER();                                                               \
    }
    if (MAXK >= 6) HGI_ENC_EDGE_COARSE(32)
    if (MAXK >= 5) HGI_ENC_EDGE_COARSE(16)
    HGI_ENC_EDGE_COARSE(8)
    HGI_ENC_EDGE_COARSE(4)
#undef HGI_ENC_EDGE_COARSE
    if (k >= 2) {
        enc_level2_fast<INTERP, IDENT, EDGE>(buf, rbuf, slut, cur.tl, W, H);
        LDS_ORDER();
    }
    enc_fine_recon<INTERP, IDENT, EDGE>(buf, rbuf, slut, cur.b, ro, odd, (int)(H - cur.tl.Y0), (int)(W - cur.tl.X0));
}

// enc_tile_fast's chain with the new last link
template <int INTERP, bool IDENT>
__device__ __forceinline__ void enc_tile_fast_recon(u8 *buf, u8 *rbuf, const u8 *slut, const TileCtx &cur, const TileSide &ro,
                                                    const v4u (&odd)[NFINE], u32 k, u32 W, u32 H)
{
#define HGI_ENC_COARSE(SUB)                                                                    \
    if (k > HGI_LOG2(SUB)) {                                                                   \
        enc_level_coarse_fast<INTERP, IDENT>(buf, rbuf, slut, SUB, cur.tl, W, H);              \
        LDS_ORDER();                                                                           \
    }
    if (MAXK >= 6) HGI_ENC_COARSE(32)
    if (MAXK >= 5) HGI_ENC_COARSE(16)
    HGI_ENC_COARSE(8)
    HGI_ENC_COARSE(4)
#undef HGI_ENC_COARSE
    if (k >= 2) {
        enc_level2_fast<INTERP, IDENT>(buf, rbuf, slut, cur.tl, W, H);
        LDS_ORDER();
    }
    enc_fine_recon<INTERP, IDENT, 0>(buf, rbuf, slut, cur.b, ro, odd);
}

// SEEDED: 0 the tile holds the pyramid, 2 the cone on the frame's own samples (k == 4).  The wave budget is k_enc_pitched's.
template <int INTERP, bool IDENT, int SEEDED>
__global__ __launch_bounds__(NL) __attribute__((amdgpu_waves_per_eu(IDENT ? HGI_ENC_WAVES_PER_EU - 1 : HGI_ENC_WAVES_PER_EU))) void k_enc_recon(
    const u8 *__restrict__ src, u8 *__restrict__ dst, u8 *__restrict__ rec, u32 k, Lut256 lut, Seeds sd, ReconPlan rp)
{
    extern __shared__ __attribute__((aligned(16))) u8 smem[];
    const PitchedPlan &p = rp.p;
    const int nh = k >= 2 ? (int)k : 1;
    // the table at LDS offset 0 (lut_at(); launch_encode_recon checks on the host that there is no static LDS)
    u8 *slut = smem;
    u8 *buf = smem + 256 - HCOL;
    u8 *rbuf = smem + 256 + buf_bytes(nh) - RCOL;
    const u32 W = p.W, H = p.H;
    bool edge, idle;
    const Tile tl = pitched_block_tile(p, edge, idle);
    if (idle) return;
    const u8 *fr = src + (size_t)tl.frame * p.sstride;
    u8 *out = dst + (size_t)tl.frame * p.dstride;
    u8 *rout = rec + (size_t)tl.frame * rp.x.stride;
    const PitchAt at = {p.sp};
    u32 lutv = 0;
    SeedRegs seeds;
    ConeLane cone;
    // 32-bit buffer offsets on all three sides (the host launches nothing else)
    u32 rb;
    TileCtx cur = {tl, pitched_buf(fr, out, p, tl, &rb)};
    const TileSide ro = tile_side(rp.x, rout, tl, 1);
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

hipError_t launch_encode_recon(const uint8_t *img, uint8_t *grid, uint8_t *recon, const ReconPlan &rp, uint32_t k, uint32_t up,
                               int interp, const Lut256 &lut, bool ident, hipStream_t s)
{
    const TileLaunch t = tile_launch(rp.p, k, up);
    if (!t.ok) return hipErrorInvalidValue;
    return with_choices(
        [&](auto I, auto ID, auto SE) {
            return launch_tile_kernel<k_enc_recon<I, ID != 0, SE>>(t.blocks, enc_lds_bytes(t.nh), s, img, grid, recon, k, lut, t.sd, rp);
        },
        interp_choice(interp), OneOf<1, 0>{ident ? 1 : 0}, OneOf<2, 0>{t.cone ? 2 : 0});
}

}  // namespace hgi
