// Mapped decode (hgi_map_decode_dev): grids decoded straight into frames of E-byte elements, out[p] = table[decoded[p]], in one
// launch.  Each tile runs k_dec_pitched's procedure (csrc/hgi_fused_pitched_dec.hip) as it stands -- the block -> tile map, the
// staging through the read pitch, the cone, the coarse-level chain, level 2 -- and a finest pass of its own, dec_fine_map, which
// forms the two decoded rows of a task exactly as dec_fine_fast does (same registers, same pred8, same 24 byte adds), lets the
// eight lanes of a row exchange pixels through LDS so that each lane holds the pixels of 16-B pieces 128 B apart, looks every
// byte up in the 256-entry table the wave keeps in LDS and stores E pieces per row through a write descriptor of the output.  (1 + E) B/px of traffic instead of the (3 + E) B/px of a decode launch and a conversion launch.
// Buffer path only: hgi_map.hip refuses the calls whose offsets need 64 bits.
//
// LDS: the decoder's own layout (buf_bytes(nh), no offset of the included procedure moves), the table behind it, 256 * E bytes,
// loaded once per tile -- each lane one vector load of 4 * E bytes, issued with the staging loads, committed with them -- and
// behind the table 2 KiB of staging rows through which the eight lanes of a row exchange their decoded pixels, so that every
// store instruction of the wave writes whole 128-B lines.  (A lane that stores its own 16 pixels writes 16 B of every 16 * E and
// no instruction fills a line: that layout is recorded in profiles/r10_mapped_lane_stores.txt)
#define HGI_FUSED_NO_LAUNCHERS 1
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"
#pragma clang diagnostic ignored "-Wunneeded-internal-declaration"
#include "../csrc/hgi_fused_dec.hip"   // the decode direction's build settings and tile procedure, 128 x 64 tiles
#include "../csrc/hgi_fused_pitched.h"
#pragma clang diagnostic pop
#include "../companion/hgi_tile.h"
#include "hgi_map_kernels.h"

// Resident tiles per CU of a launch of 8 192 tiles and more (the dynamic LDS is padded to that: lds_for_waves).  The start is
// launch_decode_pitched's policy; a launch that writes 2-4x the bytes may want another number (sweeps: make VARIANT=_x
// EXTRA=-DHGI_MAP_WAVES=n; 0 keeps the pitched decoder's).
#ifndef HGI_MAP_WAVES
#define HGI_MAP_WAVES 0
#endif
// Waves per SIMD the kernels are compiled for (the cone two fewer, as in the decoder).  E = 4 fits the uniform decoder's 8
// (64 VGPRs): its 32 lookups of a task land in the 32 dwords the stores read.  E = 2 holds 32 half-filled dwords between the
// lookups and the packing and gets 7 (72 VGPRs).  Neither limits occupancy: the LDS of a tile (7 408 / 7 920 B at k = 4) allows
// 22 / 20 tiles per CU, 5 to 5.5 waves per SIMD.
#ifndef HGI_MAP_WAVES_PER_EU_E4
#define HGI_MAP_WAVES_PER_EU_E4 HGI_DEC_WAVES_PER_EU
#endif
#ifndef HGI_MAP_WAVES_PER_EU_E2
#define HGI_MAP_WAVES_PER_EU_E2 (HGI_DEC_WAVES_PER_EU - 1)
#endif

namespace hgi {
namespace {

// Staging rows of the finest pass: the two decoded rows of each of the NL / CH row pairs a wave works on at a time, 128 B each.
constexpr int kMapStageBytes = 2 * TW * (NL / CH);

// Sixteen decoded pixels (four packed dwords) -> their table entries, E pieces of 16 B.  All lookups are issued before the
// first result is used: one dependent LDS round trip for the lookups (the exchange in front of them is a second one).  E = 4: ds_read_b32; E = 2: ds_read_u16, two
// entries packed per dword.
template <int E>
__device__ __forceinline__ void map_lookup(const u8 *tab, v4u px, v4u (&out)[E])
{
    if (E == 4) {
        u32 el[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) el[i] = *reinterpret_cast<const u32 *>(tab + 4 * ((px[i >> 2] >> (8 * (i & 3))) & 0xFFu));
#pragma unroll
        for (int p = 0; p < E; ++p) out[p] = v4u{el[4 * p], el[4 * p + 1], el[4 * p + 2], el[4 * p + 3]};
    } else {
        u32 el[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) el[i] = *reinterpret_cast<const unsigned short *>(tab + 2 * ((px[i >> 2] >> (8 * (i & 3))) & 0xFFu));
#pragma unroll
        for (int p = 0; p < E; ++p)
            out[p] = v4u{el[8 * p] | (el[8 * p + 1] << 16), el[8 * p + 2] | (el[8 * p + 3] << 16), el[8 * p + 4] | (el[8 * p + 5] << 16),
                         el[8 * p + 6] | (el[8 * p + 7] << 16)};
    }
}

// One 16-B piece of an output row of which only the first `nb` bytes (a multiple of E) lie inside the image: the whole piece,
// or its b64 / b32 and (E = 2, odd element count) b16 parts.  There is no 1-byte case.
template <int E>
__device__ __forceinline__ void store_map_piece_edge(v4u v, __amdgpu_buffer_rsrc_t rd, u32 off, int nb)
{
    if (nb >= 16) {
        __builtin_amdgcn_raw_buffer_store_b128(v, rd, off, 0, HGI_STORE_AUX);
    } else if (nb > 0) {
        if (nb & 8) __builtin_amdgcn_raw_buffer_store_b64(v2u{v.x, v.y}, rd, off, 0, HGI_STORE_AUX);
        if (nb & 4) __builtin_amdgcn_raw_buffer_store_b32((nb & 8) ? v.z : v.x, rd, off + (u32)(nb & 8), 0, HGI_STORE_AUX);
        if (E == 2 && (nb & 2)) {
            const int d = nb >> 2;
            const u32 w = d == 0 ? v.x : d == 1 ? v.y : d == 2 ? v.z : v.w;
            __builtin_amdgcn_raw_buffer_store_b16((unsigned short)w, rd, off + (u32)(nb & 12), 0, HGI_STORE_AUX);
        }
    }
}

// The E-byte row stores of a lane's task, rows y (a) and y + 1 (b); then two wait states during which every data register stays
// allocated (store_row_pair's rule; tools/check_isa.py rule 4).  Every wide store of this unit goes through
// here.  Piece p of lane c covers bytes [128 p + 16 c, + 16) of the row's 128 * E, so the eight lanes of a row fill one whole
// 128-B line per store instruction (`voff` is the offset of the lane's piece 0).  EDGE == 2: `nbytes` of the row lie inside the
// image, counted from the lane's piece 0 -- of the piece that straddles the right edge only the elements inside are stored --
// and rows at and below the image's height not at all.
template <int E, int EDGE>
__device__ __forceinline__ void store_map_rows(const v4u (&a)[E], const v4u (&b)[E], __amdgpu_buffer_rsrc_t rd, u32 voff, u32 pitch,
                                               int nbytes, bool row0, bool row1)
{
    if (EDGE == 2) {
        const u32 v1 = voff + pitch;
#pragma unroll
        for (int p = 0; p < E; ++p) {
            const int nb = nbytes - 128 * p;
            if (row0) store_map_piece_edge<E>(a[p], rd, voff + 128 * p, nb);
            if (row1) store_map_piece_edge<E>(b[p], rd, v1 + 128 * p, nb);
        }
    } else {   // EDGE == 1: row pairs below the image are dropped by the buffer range check (even height)
#pragma unroll
        for (int p = 0; p < E; ++p) __builtin_amdgcn_raw_buffer_store_b128(a[p], rd, voff + 128 * p, 0, HGI_STORE_AUX);
#pragma unroll
        for (int p = 0; p < E; ++p) __builtin_amdgcn_raw_buffer_store_b128(b[p], rd, voff + 128 * p, pitch, HGI_STORE_AUX);
    }
    if (E == 4)
        asm volatile("s_nop 1" ::"v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(b[0]), "v"(b[1]), "v"(b[2]), "v"(b[3]));
    else
        asm volatile("s_nop 1" ::"v"(a[0]), "v"(a[1]), "v"(b[0]), "v"(b[1]));
}

// The pixels of piece p of lane c: the 16 / E pixels from (128 p + 16 c) / E of the row, read back from the wave's staging rows
// (the decoded row as packed bytes, 128 B) -- the eight lanes of a row exchange their pixels so that each store instruction
// writes whole lines.
template <int E>
__device__ __forceinline__ v4u map_row_pixels(const u8 *row, int c)
{
    v4u px;
    if (E == 4) {
#pragma unroll
        for (int p = 0; p < 4; ++p) px[p] = *reinterpret_cast<const u32 *>(row + 32 * p + 4 * c);
    } else {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const v2u t = *reinterpret_cast<const v2u *>(row + 64 * p + 8 * c);
            px[2 * p] = t.x;
            px[2 * p + 1] = t.y;
        }
    }
    return px;
}

// The finest level of dec_fine_fast -- the same arithmetic on the same registers -- then the lookups and the E-byte row stores.
template <int INTERP, int E, int EDGE>
__device__ __forceinline__ void dec_fine_map(const u8 *buf, const u8 *tab, const TileSide &mo, const v4u (&odd)[NFINE], int rows, int cols)
{
    const int lane = HGI_LANE, c8 = lane & (CH - 1);
    u8 *stg = const_cast<u8 *>(tab) + 256 * E + 2 * TW * (lane >> LCH);      // the lane's two staging rows, behind the table
    const int rp0 = fine_pair0();
    const bool last = (lane & (CH - 1)) == CH - 1;
    const u8 *r0 = buf + rp0 * S + 16 * (lane & (CH - 1));
    const u8 *h0 = buf + HCOL + rp0;
    const u32 P = __builtin_amdgcn_readfirstlane(mo.pitch);
    u32 voff = mo.base + 2 * rp0 * P + 16 * c8;
#pragma unroll
    for (int it = 0; it < NFINE; ++it, r0 += (NL / CH) * S, h0 += NL / CH, voff += 2 * (NL / CH) * P) {
        v4u E_ = *reinterpret_cast<const v4u *>(r0);
        v4u O = odd[it];
        v4u F = *reinterpret_cast<const v4u *>(r0 + S);
        // ninth corner of each lattice row: first byte of the next chunk = lane + 1, or the halo column
        u32 e16 = from_next_lane(E_.x), f16 = from_next_lane(F.x);
        const u32 he = h0[0], hf = h0[1];
        e16 = last ? he : e16;
        f16 = last ? hf : f16;
        v4u r0v, r1v;
        dec_fine_rows<INTERP>(E_, F, e16, f16, O, r0v, r1v);
        // 16 px x 2 rows as packed bytes -> the staging rows of the lane's row pair; back come the pixels of the lane's pieces
        // (dword k of `px` = piece k at E = 4, half of piece k / 2 at E = 2: map_lookup's order), then every lookup of the task,
        // then the packing, then the stores
        *reinterpret_cast<v4u *>(stg + 16 * c8) = r0v;
        *reinterpret_cast<v4u *>(stg + TW + 16 * c8) = r1v;
        LDS_ORDER();
        const v4u pa = map_row_pixels<E>(stg, c8), pb = map_row_pixels<E>(stg + TW, c8);
        LDS_ORDER();
        v4u a[E], b[E];
        map_lookup<E>(tab, pa, a);
        map_lookup<E>(tab, pb, b);
        const int y = 2 * (rp0 + it * (NL / CH));
        store_map_rows<E, EDGE>(a, b, mo.r, voff, P, cols * E - 16 * c8, y < rows, y + 1 < rows);
    }
}

// dec_tile_fast / dec_tile_edge's level chain, then the mapped finest level.  EDGE == 0: the tile body lies inside the image;
// 1: full width inside, even height (no column logic, the range check drops the rows below the image); 2: any ragged tile.
template <int INTERP, int E, int EDGE>
__device__ __forceinline__ void dec_tile_map(u8 *buf, const u8 *tab, Tile tl, const TileSide &mo, const v4u (&odd)[NFINE], u32 k, u32 W, u32 H)
{
    dec_chain<INTERP, EDGE>(buf, tl, k, W, H);
    dec_fine_map<INTERP, E, EDGE>(buf, tab, mo, odd, (int)(H - tl.Y0), (int)(W - tl.X0));
}

// A lane's 4 * E bytes of the table: one vector load, at any alignment of the table.
template <int E>
struct TabLane {
    u32 w[E];
};

constexpr int map_waves_per_eu(int seeded, int e)
{
    return (e == 4 ? HGI_MAP_WAVES_PER_EU_E4 : HGI_MAP_WAVES_PER_EU_E2) - (seeded == 2 ? 2 : 0);
}

// One block (= one wave) per tile.  SEEDED: 0 = the pyramid fits the tile (k = levels <= 5); 2 = the cone (k == 4, sd.up levels
// above the tile, rebuilt from the frame's own base samples through the pitch).  E: bytes per output element.
template <int INTERP, int SEEDED, int E>
__global__ __launch_bounds__(NL) __attribute__((amdgpu_waves_per_eu(map_waves_per_eu(SEEDED, E)))) void k_dec_map(
    const u8 *__restrict__ src, const u8 *__restrict__ tabg, u8 *__restrict__ dst, u32 k, Seeds sd, MapPlan mp)
{
    extern __shared__ __attribute__((aligned(16))) u8 smem[];
    const PitchedPlan &p = mp.p;
    const int nh = k >= 2 ? (int)k : 1;
    u8 *buf = smem - HCOL;
    u8 *tab = smem + buf_bytes(nh);      // behind the decoder's layout (launch_decode_map checks that there is no static LDS)
    const u32 W = p.W, H = p.H;
    bool edge, idle;
    const Tile tl = pitched_block_tile(p, edge, idle);
    if (idle) return;
    const u8 *fr = src + (size_t)tl.frame * p.sstride;
    u8 *out = dst + (size_t)tl.frame * mp.x.stride;
    const PitchAt at = {p.sp};
    // 32-bit buffer offsets on both sides (the host launches nothing else)
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(fr), 0, p.srec, 0x00020000);
    const u32 rb = __builtin_amdgcn_readfirstlane(tl.Y0 * p.sp32 + tl.X0);
    const TileSide mo = tile_side(mp.x, out, tl, E);
    SeedRegs seeds;
    ConeLane cone;
    Stage st;
    TabLane<E> tv;
    if (!edge) {
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

hipError_t launch_decode_map(const uint8_t *grid, const void *table, void *out, const MapPlan &mp, uint32_t elem, uint32_t k,
                             uint32_t up, int interp, hipStream_t s)
{
    const PitchedPlan &p = mp.p;
    const TileLaunch t = tile_launch(p, k, up);
    if (!t.ok || (elem != 2 && elem != 4)) return hipErrorInvalidValue;
    // resident tiles per CU: the decoders' policy on this launch's tile count, unless this unit was built with a number of its
    // own for launches of 8 192 tiles and more
    const u64 tiles = (u64)p.nf + p.nedge;
    const int waves = tiles >= 8192 && HGI_MAP_WAVES > 0 ? HGI_MAP_WAVES : dec_resident_tiles(tiles, p.W, k, t.cone);
    const size_t lds = lds_for_waves((size_t)buf_bytes(t.nh) + 256 * (size_t)elem + kMapStageBytes, waves);   // the decoder's, the table and the staging rows behind it
    const u8 *tab = static_cast<const u8 *>(table);
    u8 *dst = static_cast<u8 *>(out);
    return with_choices(
        [&](auto I, auto SE, auto EL) { return launch_tile_kernel<k_dec_map<I, SE, EL>>(t.blocks, lds, s, grid, tab, dst, k, t.sd, mp); },
        interp_choice(interp), OneOf<2, 0>{t.cone ? 2 : 0}, OneOf<4, 2>{(int)elem});
}

}  // namespace hgi
