// Region decode (hgi_decode_region_u8_dev): the window [x0, x0 + w) x [y0, y0 + h) of every frame of a batch, decoded by the
// tiles of the frame's own 128 x 64 lattice that intersect it and by no others.
//
// A pixel depends only on coarser pixels to its right and below it, and the fused decoder already decodes every tile on its
// own: the halo is recomputed inside the tile, the levels above a six- to eight-level tile are rebuilt from the cone, deeper
// pyramids start from the stride-256 lattice plane.  So a tile at the same origin, staged from the same grid
// bytes, runs exactly the code the full decode runs -- k_dec_tiles' tile procedure as it stands: staging, the cone / seeds,
// dec_tile_fast -- and produces the same bytes; what is new is the tile list (the cover of the window) and the finest
// level's store, which writes into a window-sized output with its own pitch and is clipped on all four sides.
//   * Tiles wholly inside the window take dec_tile_fast unchanged, its 16-B row stores addressed through a descriptor of the
//     window: base (Y0 - y0) * pitch + (X0 - x0), pitch = the output's.
//   * Tiles on the window's border and ragged tiles of the frame (right / bottom edge: the buffer range check and the lane
//     masks of the ragged staging supply the out-of-image zeros) run the same level chain and store through
//     store_rows_window: whole 16-B chunks of whole row pairs as before, the chunks cut by the window's left or right edge
//     dword- or byte-wise, rows above or below the window not at all.
//   * Frames whose byte offsets do not fit 32 bits (and the knobs build's HGI_FORCE_CHECKED) take the byte-checked path of
//     k_dec_tiles with a finest level that stores the window's bytes only.
// Cost: the tiles of the cover -- ceil-aligned to 128 x 64 -- plus, from nine levels, the lattice launch over the whole frame's
// stride-256 plane (w * h / 65536 points).
#define HGI_FUSED_NO_LAUNCHERS 1
#include "hgi_fused_dec.hip"   // the decode direction's build settings and tile procedure, 128 x 64 tiles
#include "hgi_dec_chain.h"

namespace hgi {
namespace {

// The cover: tile columns cx0 .. cx0 + ncx - 1 and rows cy0 .. cy0 + ncy - 1 of the frame's lattice.  The first ix x iy of
// them are interior (body inside the image, buffer path allowed: the same test as fused_geom's); the others -- the cover's
// part right of full_x, then its part below full_y -- are the ragged / checked ones, dispatched first like block_role's.
struct Region {
    u32 x0, y0, rw, rh;          // the window, frame coordinates
    u32 cx0, cy0, ncx, ncy;
    u32 ix, iy;
    u32 ipf, epf;                // interior / other tiles per frame
    u32 nf, nedge;               // ... over the batch
    FastDiv fd_ix, fd_ipf;
    u32 pitch, span;             // output pitch and bytes of one frame's window, (rh - 1) * pitch + rw (buffer path: < 2^32)
    u64 opitch, ostride;         // the same pitch in 64 bits (checked path), bytes between the frames' windows
};

__device__ __forceinline__ Tile region_tile(const Region &rg, bool &edge, bool &idle)
{
    const u32 b = blockIdx.x, ne8 = (rg.nedge + 7u) & ~7u;
    Tile tl;
    u32 tx, ty;
    edge = b < ne8;
    idle = edge && b >= rg.nedge;
    if (edge) {
        const u32 e = idle ? 0u : b;
        tl.frame = e / rg.epf;
        u32 i = e - tl.frame * rg.epf;
        const u32 right = (rg.ncx - rg.ix) * rg.ncy;      // cover columns right of the interior ones, every cover row
        if (i < right) {
            const u32 w = rg.ncx - rg.ix;
            ty = i / w;
            tx = rg.ix + (i - ty * w);
        } else {                                          // interior columns, rows below the interior ones
            i -= right;
            ty = rg.iy + i / rg.ix;
            tx = i % rg.ix;
        }
    } else {
        // interior tiles frame by frame, row-major, the list dealt to the XCDs in contiguous eighths (range_first): tiles that
        // share halo lines meet in one L2
        const u32 fb = b - ne8;
        const u32 t = range_first(rg.nf, fb & 7u) + (fb >> 3);
        tl.frame = fdiv(t, rg.fd_ipf);
        const u32 r = t - tl.frame * rg.ipf;
        ty = fdiv(r, rg.fd_ix);
        tx = r - ty * rg.ix;
    }
    tl.X0 = (rg.cx0 + tx) * TW;
    tl.Y0 = (rg.cy0 + ty) * TH;
    return tl;
}

// The part of a tile that lies inside the window, in tile coordinates: columns [lo, hi), rows [ylo, yhi).
struct Clip {
    int lo, hi, ylo, yhi;
};

__device__ __forceinline__ Clip tile_clip(const Region &rg, Tile tl)
{
    Clip c;
    c.lo = rg.x0 > tl.X0 ? (int)(rg.x0 - tl.X0) : 0;
    c.ylo = rg.y0 > tl.Y0 ? (int)(rg.y0 - tl.Y0) : 0;
    const u32 xe = rg.x0 + rg.rw - tl.X0, ye = rg.y0 + rg.rh - tl.Y0;     // > 0: the tile intersects the window
    c.hi = xe < (u32)TW ? (int)xe : TW;
    c.yhi = ye < (u32)TH ? (int)ye : TH;
    return c;
}

// The row pair of a lane, clipped to the window: bytes [clo, chi) of the lane's 16-B chunk, rows row0 / row1.  Whole chunks of
// whole pairs go through store_row_pair; one row of a whole chunk as two 8-B stores; a chunk the window's left or right edge
// cuts as its whole dwords and the bytes around them.  Offsets are formed in 32-bit arithmetic and only for bytes inside the
// window, which all lie in [0, span).  The data registers are held like in store_row_pair.
__device__ __forceinline__ void store_rows_window(v4u r0, v4u r1, __amdgpu_buffer_rsrc_t rd, u32 voff, u32 pitch, int clo, int chi,
                                                  bool row0, bool row1)
{
    const bool whole = clo <= 0 && chi >= 16;
    const u32 v1 = voff + pitch;
    if (whole && row0 && row1) {
        store_row_pair(r0, r1, rd, voff, pitch);
    } else if (whole) {
        if (row0) {
            __builtin_amdgcn_raw_buffer_store_b64(v2u{r0.x, r0.y}, rd, voff, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b64(v2u{r0.z, r0.w}, rd, voff + 8, 0, 0);
        }
        if (row1) {
            __builtin_amdgcn_raw_buffer_store_b64(v2u{r1.x, r1.y}, rd, v1, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b64(v2u{r1.z, r1.w}, rd, v1 + 8, 0, 0);
        }
    } else if (clo < 16 && chi > 0 && (row0 || row1)) {
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const u32 w0 = d == 0 ? r0.x : d == 1 ? r0.y : d == 2 ? r0.z : r0.w;
            const u32 w1 = d == 0 ? r1.x : d == 1 ? r1.y : d == 2 ? r1.z : r1.w;
            if (4 * d >= clo && 4 * d + 4 <= chi) {
                if (row0) __builtin_amdgcn_raw_buffer_store_b32(w0, rd, voff + 4 * d, 0, 0);
                if (row1) __builtin_amdgcn_raw_buffer_store_b32(w1, rd, v1 + 4 * d, 0, 0);
            } else if (4 * d + 4 > clo && 4 * d < chi) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (4 * d + j < clo || 4 * d + j >= chi) continue;
                    if (row0) __builtin_amdgcn_raw_buffer_store_b8((u8)(w0 >> (8 * j)), rd, voff + 4 * d + j, 0, 0);
                    if (row1) __builtin_amdgcn_raw_buffer_store_b8((u8)(w1 >> (8 * j)), rd, v1 + 4 * d + j, 0, 0);
                }
            }
        }
    }
    asm volatile("s_nop 1" ::"v"(r0), "v"(r1));
}

// The finest level of dec_fine_fast -- the same arithmetic on the same registers -- with the window's store.  `base` is the
// output offset of the tile's origin (Y0 - y0) * pitch + (X0 - x0), modulo 2^32 (negative for tiles that start outside).
template <int INTERP>
__device__ __forceinline__ void dec_fine_region(const u8 *buf, __amdgpu_buffer_rsrc_t rd, u32 base, u32 pitch, const v4u (&odd)[NFINE],
                                                Clip cl)
{
    const int lane = HGI_LANE;
    const int rp0 = fine_pair0();
    const bool last = (lane & (CH - 1)) == CH - 1;
    const int c16 = 16 * (lane & (CH - 1));
    const u8 *r0 = buf + rp0 * S + c16;
    const u8 *h0 = buf + HCOL + rp0;
#pragma unroll
    for (int it = 0; it < NFINE; ++it, r0 += (NL / CH) * S, h0 += NL / CH) {
        v4u E = *reinterpret_cast<const v4u *>(r0);
        v4u O = odd[it];
        v4u F = *reinterpret_cast<const v4u *>(r0 + S);
        u32 e16 = from_next_lane(E.x), f16 = from_next_lane(F.x);
        const u32 he = h0[0], hf = h0[1];
        e16 = last ? he : e16;
        f16 = last ? hf : f16;
        v4u r0v, r1v;
        dec_fine_rows<INTERP>(E, F, e16, f16, O, r0v, r1v);
        const int y = 2 * (rp0 + it * (NL / CH));
        const u32 voff = base + (u32)y * pitch + (u32)c16;
        store_rows_window(r0v, r1v, rd, voff, __builtin_amdgcn_readfirstlane(pitch), cl.lo - c16, cl.hi - c16,
                          y >= cl.ylo && y < cl.yhi, y + 1 >= cl.ylo && y + 1 < cl.yhi);
    }
}

// dec_tile_fast / dec_tile_edge's level chain, then the clipped finest level.  EDGE == 0: the tile body lies inside the image;
// EDGE == 2: any ragged tile (dec_level2_fast keeps the out-of-image lattice points zero).
template <int INTERP, int EDGE>
__device__ __forceinline__ void dec_tile_region(u8 *buf, Tile tl, __amdgpu_buffer_rsrc_t rd, u32 base, u32 pitch, Clip cl,
                                                const v4u (&odd)[NFINE], u32 k, u32 W, u32 H)
{
    dec_chain<INTERP, EDGE>(buf, tl, k, W, H);
    dec_fine_region<INTERP>(buf, rd, base, pitch, odd, cl);
}

// finest level of the byte-checked path (dec_fine_generic's arithmetic), storing the window's bytes only; 64-bit addressing
// (the window by value: a reference to the kernel argument would be a copy on the stack)
template <int INTERP>
__device__ __noinline__ void dec_fine_generic_region(const u8 *buf, const u8 *__restrict__ fr, u8 *__restrict__ out, Tile tl, u32 W,
                                                     u32 H, u32 x0, u32 y0, u32 rw, u32 rh, u64 opitch, bool aligned)
{
    for (int i = HGI_LANE; i < (TH / 2) * CH; i += NL) {
        const int z = i >> LCH, y = 2 * z, x = 16 * (i & (CH - 1));
        const u32 gx = tl.X0 + x, gy = tl.Y0 + y;
        if (gx >= x0 + rw || gx + 16 <= x0 || gy >= y0 + rh || gy + 2 <= y0) continue;
        const u8 *r0 = buf + z * S + x;
        uint4 E = *reinterpret_cast<const uint4 *>(r0);
        uint4 O = load16(fr, W, H, gx, gy + 1, aligned);
        uint4 F = *reinterpret_cast<const uint4 *>(r0 + S);
        u32 e16 = x + 16 < TW ? r0[16] : buf[HCOL + z], f16 = x + 16 < TW ? r0[S + 16] : buf[HCOL + z + 1];
        uint2 c, fl;
        c.x = __builtin_amdgcn_perm(E.y, E.x, 0x06040200u);
        c.y = __builtin_amdgcn_perm(E.w, E.z, 0x06040200u);
        fl.x = __builtin_amdgcn_perm(F.y, F.x, 0x06040200u);
        fl.y = __builtin_amdgcn_perm(F.w, F.z, 0x06040200u);
        u32 P0, P1;
        pred8<INTERP>(c, e16, fl, f16, P0, P1);
        u32 pp0 = __builtin_amdgcn_perm(P0, P0, 0x01010000u), pp1 = __builtin_amdgcn_perm(P0, P0, 0x03030202u);
        u32 pp2 = __builtin_amdgcn_perm(P1, P1, 0x01010000u), pp3 = __builtin_amdgcn_perm(P1, P1, 0x03030202u);
        const u32 odd = 0xFF00FF00u;
        const u32 o0[4] = {add4(E.x, pp0 & odd), add4(E.y, pp1 & odd), add4(E.z, pp2 & odd), add4(E.w, pp3 & odd)};
        const u32 o1[4] = {add4(O.x, pp0), add4(O.y, pp1), add4(O.z, pp2), add4(O.w, pp3)};
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const u32 px = gx + j;
            if (px < x0 || px >= x0 + rw) continue;
            u8 *col = out + (px - x0);
            if (gy >= y0 && gy < y0 + rh) col[(size_t)(gy - y0) * opitch] = (u8)(o0[j >> 2] >> (8 * (j & 3)));
            if (gy + 1 >= y0 && gy + 1 < y0 + rh) col[(size_t)(gy + 1 - y0) * opitch] = (u8)(o1[j >> 2] >> (8 * (j & 3)));
        }
    }
}

// One block (= one wave) per tile of the cover, ONE launch per batch.  SEEDED: 0 = the pyramid fits the tile; 2 = the cone
// (k == 4, sd.up levels above the tile; from nine levels on the stride-256 lattice planes).  The wave budget is k_dec_tiles'.
template <int INTERP, int SEEDED>
__global__ __launch_bounds__(NL) __attribute__((amdgpu_waves_per_eu(SEEDED == 2 ? HGI_DEC_WAVES_PER_EU - 2 : HGI_DEC_WAVES_PER_EU))) void k_dec_region(
    const u8 *__restrict__ src, u8 *__restrict__ dst, Frames f, u32 k, Seeds sd, Region rg, u32 aligned)
{
    extern __shared__ __attribute__((aligned(16))) u8 smem[];
    const int nh = k >= 2 ? (int)k : 1;
    u8 *buf = smem - HCOL;
    const u32 W = f.width, H = f.height;
    bool edge, idle;
    const Tile tl = region_tile(rg, edge, idle);
    if (idle) return;
    const u8 *fr = src + (size_t)tl.frame * f.frame_stride;
    u8 *out = dst + (size_t)tl.frame * rg.ostride;
    const Clip cl = tile_clip(rg, tl);
    SeedRegs seeds;
    ConeLane cone;
    if (aligned & 2u) {   // 32-bit buffer offsets on both sides: buffer staging, the check-free levels
        const TileCtx cur = {tl, make_buf(fr, out, W, H, tl, (aligned & 4u) ? 3u : 0u)};
        Buf bo = cur.b;       // the store side: the frame's window
        bo.rd = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(out), 0, rg.span, 0x00020000);
        bo.W = rg.pitch;
        bo.base = __builtin_amdgcn_readfirstlane((tl.Y0 - rg.y0) * rg.pitch + (tl.X0 - rg.x0));
        Stage st;
        if (!edge) {
            stage_issue<false>(st, cur.b, tl, (int)k, nh);
            if (SEEDED == 2) cone = cone_issue<false>(fr, W, H, sd, tl);
            stage_commit<false>(buf, nullptr, st, nh);
            LDS_ORDER();
            if (HGI_ODD_LATE) stage_issue_odd(st, cur.b);
        } else {
            if (SEEDED == 2) cone = cone_issue<false>(fr, W, H, sd, tl);
            stage_issue<true, true>(st, cur.b, tl, (int)k, nh);
            stage_commit<false>(buf, nullptr, st, nh);
            LDS_ORDER();
        }
        if (SEEDED == 2) seeds = cone_finish<INTERP, false, true>(cone, buf, nullptr, sd.up, nullptr);
        LDS_ORDER();
        if (SEEDED) dec_seed_commit(buf, seeds, k);
        if (edge)
            dec_tile_region<INTERP, 2>(buf, tl, bo.rd, bo.base, bo.W, cl, st.o, k, W, H);
        else if (cl.lo == 0 && cl.hi == TW && cl.ylo == 0 && cl.yhi == TH)
            dec_tile_fast<INTERP>(buf, TileCtx{tl, bo}, st.o, k, W, H);      // the whole tile is in the window
        else
            dec_tile_region<INTERP, 0>(buf, tl, bo.rd, bo.base, bo.W, cl, st.o, k, W, H);
        return;
    }
    // frames whose byte offsets (or windows whose output span) do not fit 32 bits: every access checked, 64-bit addressing
    if (SEEDED == 2) cone = cone_issue<false>(fr, W, H, sd, tl);
    stage_tile_generic(buf, fr, W, H, tl, nh, (aligned & 1u) != 0);
    LDS_ORDER();
    if (SEEDED == 2) seeds = cone_finish<INTERP, false, true>(cone, buf, nullptr, sd.up, nullptr);
    if (SEEDED) dec_seed_commit(buf, seeds, k);
    for (int s = 1 << (k - 1); s >= 2; s >>= 1) {
        dec_cells<INTERP, true>(buf, s, tl, W, H);
        dec_halo_cells<INTERP>(buf, s, tl, W, H);
        LDS_ORDER();
    }
    dec_fine_generic_region<INTERP>(buf, fr, out, tl, W, H, rg.x0, rg.y0, rg.rw, rg.rh, rg.opitch, (aligned & 1u) != 0);
}

}  // namespace

hipError_t launch_decode_region(const uint8_t *grid, uint8_t *out, const Frames &f, const RegionRect &rr, uint32_t k, int interp,
                                const Seeds *seeds, hipStream_t s)
{
    // the grid side is the full decode's: which tiles are interior, whether the buffer path is allowed, how loads are aligned
    FusedGeom r = fused_geom(grid, out, f, 0);
    if (!r.ok || k < 1 || k > (u32)MAXK || rr.width == 0 || rr.height == 0) return hipErrorInvalidValue;
    if ((u64)rr.x0 + rr.width > f.width || (u64)rr.y0 + rr.height > f.height) return hipErrorInvalidValue;
    if (seeds && k < (uint32_t)kSeededMinLevels) return hipErrorInvalidValue;
    const bool cone = seeds && seeds->up != 0;
    if (seeds && (!cone || k != 4 || seeds->up > (u32)kConeMaxUp)) return hipErrorInvalidValue;   // (no seed-plane route here)
    Region rg;
    rg.x0 = rr.x0;
    rg.y0 = rr.y0;
    rg.rw = rr.width;
    rg.rh = rr.height;
    rg.opitch = rr.out_pitch;
    rg.ostride = rr.out_frame_stride;
    const StoreSide st = store_side_32(rr.height, rr.width, rr.out_pitch);      // one frame's window addressed with 32 bits
    if (!st.ok) {
        r.aligned &= 1u;                    // every tile through the byte-checked path
        r.g.full_x = r.g.full_y = 0;
    }
    rg.pitch = st.ok ? (u32)st.pitch : 0u;
    rg.span = st.ok ? (u32)st.span : 0u;
    rg.cx0 = rr.x0 / TW;
    rg.cy0 = rr.y0 / TH;
    const u32 cx1 = (rr.x0 + rr.width - 1) / TW + 1, cy1 = (rr.y0 + rr.height - 1) / TH + 1;
    rg.ncx = cx1 - rg.cx0;
    rg.ncy = cy1 - rg.cy0;
    rg.ix = r.g.full_x > rg.cx0 ? (cx1 < r.g.full_x ? cx1 : r.g.full_x) - rg.cx0 : 0u;
    rg.iy = r.g.full_y > rg.cy0 ? (cy1 < r.g.full_y ? cy1 : r.g.full_y) - rg.cy0 : 0u;
    if (rg.ix == 0 || rg.iy == 0) rg.ix = rg.iy = 0;
    rg.ipf = rg.ix * rg.iy;
    rg.epf = rg.ncx * rg.ncy - rg.ipf;
    const u64 nf = (u64)rg.ipf * f.batch, ne = (u64)rg.epf * f.batch;
    if (nf + ne + 8 >= (1ull << 31)) return hipErrorInvalidValue;
    rg.nf = (u32)nf;
    rg.nedge = (u32)ne;
    rg.fd_ix = make_fastdiv(rg.ix ? rg.ix : 1u);
    rg.fd_ipf = make_fastdiv(rg.ipf ? rg.ipf : 1u);
    Seeds sd = seeds ? *seeds : Seeds{nullptr, nullptr, 0, 0, 0, 0};
    const int nh = k >= 2 ? (int)k : 1;
    const size_t lds = lds_for_waves((size_t)buf_bytes(nh), dec_resident_tiles(nf + ne, f.width, k, seeds != nullptr));
    const dim3 blocks(((rg.nedge + 7u) & ~7u) + rg.nf);
    return with_choices([&](auto I, auto SE) { return launch_tile_kernel<k_dec_region<I, SE>>(blocks, lds, s, grid, out, f, k, sd, rg, r.aligned); },
                        interp_choice(interp), OneOf<2, 0>{cone ? 2 : 0});
}

}  // namespace hgi
