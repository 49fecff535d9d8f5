// Device side of the pitched kernels, shared by both directions (included behind hgi_fused_dec.hip / hgi_fused_enc.hip):
// staging in which the READ pitch and the image WIDTH are two numbers, and the byte-checked path with a pitch on each side.
// The store side needs nothing new: the fine levels address the output through Buf's `W` and `base`, which the pitched kernels
// fill with the WRITE pitch and Y0 * write pitch + X0 (as region and scaled decode do), while every test against the image in
// the tile procedure takes the width and height it is handed.
#pragma once
#include "hgi_pitched.h"

namespace hgi {
namespace {

// byte (x, y) of a frame whose rows lie `p` bytes apart (cone_issue's addressing hook)
struct PitchAt {
    u64 p;
    __device__ __forceinline__ size_t operator()(size_t x, size_t y, u32) const { return y * p + x; }
};

__device__ __forceinline__ Tile pitched_block_tile(const PitchedPlan &p, bool &edge, bool &idle)
{
    const PitchedTile t = pitched_tile(p, blockIdx.x);
    edge = t.edge;
    idle = t.idle;
    Tile tl;
    tl.frame = __builtin_amdgcn_readfirstlane(t.frame);
    tl.X0 = __builtin_amdgcn_readfirstlane(t.X0);
    tl.Y0 = __builtin_amdgcn_readfirstlane(t.Y0);
    return tl;
}

// The descriptors of a frame and the store side's addressing; *rb = offset of the tile's origin on the read side.
__device__ __forceinline__ Buf pitched_buf(const u8 *fr, u8 *out, const PitchedPlan &p, Tile tl, u32 *rb)
{
    Buf b;
    b.rs = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(fr), 0, p.srec, 0x00020000);
    b.rd = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(out), 0, p.drec, 0x00020000);
    b.W = p.dp32;
    b.base = __builtin_amdgcn_readfirstlane(tl.Y0 * p.dp32 + tl.X0);
    *rb = __builtin_amdgcn_readfirstlane(tl.Y0 * p.sp32 + tl.X0);
    return b;
}

// stage_issue with the rows `P` bytes apart: addresses step by P, every test against the image uses W.  Rows at and below the
// image's height start at or beyond the descriptor's records and read 0; the bytes right of a row's end -- the gap, foreign
// data -- are never asked for by an interior tile (its chunks and halo columns are tested against W) and are masked out of the
// chunk that straddles the edge of a ragged one, exactly as a packed frame's next-row pixels are.
template <bool RAGGED, bool ODD_CHECKED = false>
__device__ __forceinline__ void pitched_issue(Stage &st, __amdgpu_buffer_rsrc_t rs, u32 rb, u32 pitch, u32 W, Tile tl, int k, int nh)
{
    const int lane = HGI_LANE, c = lane & (CH - 1), r = lane >> LCH;
    const u32 P = __builtin_amdgcn_readfirstlane(pitch);   // soffset operands must be provably uniform
    const u32 voff = rb + 2 * r * P + 16 * c;                          // even rows 2 * (r + 8 j)
    const u32 vodd = rb + (2 * fine_pair0() + 1) * P + 16 * c;         // odd rows 2 * (pair0 + 8 it) + 1
    const bool cin = tl.X0 + 16 * c < W;
    const bool narrow = RAGGED && tl.X0 + TW > W;   // wave-uniform: this tile straddles the right edge
    const v4u cm = narrow ? chunk_mask((int)W - (int)(tl.X0 + 16 * c)) : v4u{~0u, ~0u, ~0u, ~0u};
#pragma unroll
    for (int j = 0; j < TH / 16; ++j) {
        st.e[j] = v4u{0, 0, 0, 0};
        if (RAGGED) {
            if (cin) st.e[j] = __builtin_amdgcn_raw_buffer_load_b128(rs, voff + j * 16 * P, 0, 0);
            if (narrow) st.e[j] &= cm;
        } else {
            st.e[j] = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, j * 16 * P, HGI_LOAD_AUX);
        }
    }
#pragma unroll
    for (int j = 0; j < NFINE; ++j) {
        st.o[j] = v4u{0, 0, 0, 0};
        if (RAGGED && ODD_CHECKED && cin) st.o[j] = __builtin_amdgcn_raw_buffer_load_b128(rs, vodd + j * 16 * P, 0, HGI_ODD_LOAD_AUX);
        if (narrow) st.o[j] &= cm;
    }
    st.hv = v4u{0, 0, 0, 0};
    if (lane < nh * CH && cin) st.hv = __builtin_amdgcn_raw_buffer_load_b128(rs, rb + (TH + hoff(r)) * P + 16 * c, 0, 0);
    if (narrow) st.hv &= cm;
    const int hy = lane < TH / 2 ? 2 * lane : TH + hoff(lane - TH / 2);
    const u32 xo = rb + hy * P + TW;
    const u32 xr = tl.X0 + TW;              // first column right of the tile
    st.x0 = v3u{0, 0, 0};
    st.d16 = st.d32 = st.d64 = 0;
    st.zero4 = st.zero8 = false;
    if (lane < TH / 2 + nh) {
        if (xr < W) st.x0 = __builtin_amdgcn_raw_buffer_load_b96(rs, xo, 0, 0);
        st.zero4 = xr + 4 >= W;     // cleared at commit (stage_commit), like stage_issue's
        st.zero8 = xr + 8 >= W;
        if (k >= 4 && !(hy & 15) && xr + 16 < W) st.d16 = __builtin_amdgcn_raw_buffer_load_b32(rs, xo + 16, 0, 0);
        if (k >= 5 && !(hy & 31) && xr + 32 < W) st.d32 = __builtin_amdgcn_raw_buffer_load_b32(rs, xo + 32, 0, 0);
        if (k >= 6 && !(hy & 63) && xr + 64 < W) st.d64 = __builtin_amdgcn_raw_buffer_load_b32(rs, xo + 64, 0, 0);
    }
}

// The odd rows of an interior tile, requested after the even rows are committed (stage_issue_odd).
__device__ __forceinline__ void pitched_issue_odd(Stage &st, __amdgpu_buffer_rsrc_t rs, u32 rb, u32 pitch)
{
    const int c = HGI_LANE & (CH - 1);
    const u32 P = __builtin_amdgcn_readfirstlane(pitch);
    const u32 vodd = rb + (2 * fine_pair0() + 1) * P + 16 * c;
#pragma unroll
    for (int j = 0; j < NFINE; ++j) st.o[j] = __builtin_amdgcn_raw_buffer_load_b128(rs, vodd, j * 16 * P, HGI_ODD_LOAD_AUX);
}

// ---- byte-checked path: 64-bit addressing, every access tested against the image, a pitch on each side ---------------------
// 16 image bytes at (gx, gy); zero beyond the image.  A chunk inside the row is one 16-B access at any alignment (load16).
__device__ __forceinline__ uint4 pitched_load16(const u8 *__restrict__ fr, u64 pitch, u32 W, u32 H, u32 gx, u32 gy)
{
    uint4 v = make_uint4(0, 0, 0, 0);
    if (gy < H && gx < W) {
        const u8 *p = fr + (size_t)gy * pitch + gx;
        if (gx + 16 <= W) {
            __builtin_memcpy(&v, p, 16);
        } else {
            u32 w[4] = {0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (gx + j < W) w[j >> 2] |= (u32)p[j] << (8 * (j & 3));
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
    }
    return v;
}

__device__ __forceinline__ void pitched_store16(u8 *__restrict__ out, u64 pitch, u32 W, u32 gx, u32 gy, uint4 v)
{
    u8 *p = out + (size_t)gy * pitch + gx;
    if (gx + 16 <= W) {
        __builtin_memcpy(p, &v, 16);
    } else {
        u32 w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (gx + j < W) p[j] = (u8)(w[j >> 2] >> (8 * (j & 3)));
    }
}

// stage_tile_generic through the read pitch
__device__ __noinline__ void stage_pitched_generic(u8 *buf, const u8 *__restrict__ fr, u64 pitch, u32 W, u32 H, Tile tl, int nh)
{
    const int lane = HGI_LANE;
    for (int i = lane; i < (TH / 2 + nh) * CH; i += NL) {      // even rows and halo rows only
        const int rr = i >> LCH, c = i & (CH - 1);
        const int y = rr < TH / 2 ? 2 * rr : TH + hoff(rr - TH / 2);
        *reinterpret_cast<uint4 *>(buf + rr * S + 16 * c) = pitched_load16(fr, pitch, W, H, tl.X0 + 16 * c, tl.Y0 + y);
    }
    for (int i = lane; i < 8 * (TH / 2 + nh); i += NL) {       // halo columns TW + {0,4,8,..}: byte gathers
        const int hc = i & 7, rr = i >> 3;
        if (hc >= nh) continue;
        const int off = hoff(hc);
        const int y = rr < TH / 2 ? 2 * rr : TH + hoff(rr - TH / 2);
        if (rr < TH / 2 && (y & ((off ? off : 2) - 1))) continue;
        const u32 gx = tl.X0 + TW + off, gy = tl.Y0 + y;
        buf[HCOL + hc * HP + rr] = (gx < W && gy < H) ? fr[(size_t)gy * pitch + gx] : (u8)0;
    }
}

#ifdef HGI_FUSED_DECODE
// dec_fine_generic: odd rows through the read pitch, stores through the write pitch
template <int INTERP>
__device__ __noinline__ void dec_fine_generic_pitched(const u8 *buf, const u8 *__restrict__ fr, u8 *__restrict__ out, Tile tl, u32 W,
                                                      u32 H, u64 sp, u64 dp)
{
    for (int i = HGI_LANE; i < (TH / 2) * CH; i += NL) {
        const int z = i >> LCH, y = 2 * z, x = 16 * (i & (CH - 1));
        const u32 gx = tl.X0 + x, gy = tl.Y0 + y;
        if (gx >= W || gy >= H) continue;
        const u8 *r0 = buf + z * S + x;
        uint4 E = *reinterpret_cast<const uint4 *>(r0);
        uint4 O = pitched_load16(fr, sp, W, H, gx, gy + 1);     // odd rows never enter LDS
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
        uint4 o0 = make_uint4(add4(E.x, pp0 & odd), add4(E.y, pp1 & odd), add4(E.z, pp2 & odd), add4(E.w, pp3 & odd));
        uint4 o1 = make_uint4(add4(O.x, pp0), add4(O.y, pp1), add4(O.z, pp2), add4(O.w, pp3));
        pitched_store16(out, dp, W, gx, gy, o0);
        if (gy + 1 < H) pitched_store16(out, dp, W, gx, gy + 1, o1);
    }
}
#endif

#ifdef HGI_FUSED_ENCODE
// enc_fine_generic: odd rows through the read pitch, stores through the write pitch
template <int INTERP, bool IDENT>
__device__ __forceinline__ void enc_fine_generic_pitched(const u8 *buf, const u8 *rbuf, const u8 *slut, const u8 *__restrict__ fr,
                                                         u8 *__restrict__ out, Tile tl, u32 W, u32 H, u64 sp, u64 dp)
{
    for (int i = HGI_LANE; i < (TH / 2) * CH; i += NL) {
        const int y = 2 * (i >> LCH), x = 16 * (i & (CH - 1));
        const u32 gx = tl.X0 + x, gy = tl.Y0 + y;
        if (gx >= W || gy >= H) continue;
        const u8 *r0 = buf + (y >> 1) * S + x;
        const u8 *c0 = rbuf + (y >> 1) * S2 + (x >> 1);
        uint4 E = *reinterpret_cast<const uint4 *>(r0);
        uint4 O = pitched_load16(fr, sp, W, H, gx, gy + 1);     // odd rows never enter LDS
        uint2 c = *reinterpret_cast<const uint2 *>(c0);
        uint2 fl = *reinterpret_cast<const uint2 *>(c0 + S2);
        u32 c8 = x + 16 < TW ? c0[8] : rbuf[RCOL + (y >> 1)], f8 = x + 16 < TW ? c0[S2 + 8] : rbuf[RCOL + (y >> 1) + 1];
        u32 P0, P1;
        pred8<INTERP>(c, c8, fl, f8, P0, P1);
        u32 pp0 = __builtin_amdgcn_perm(P0, P0, 0x01010000u), pp1 = __builtin_amdgcn_perm(P0, P0, 0x03030202u);
        u32 pp2 = __builtin_amdgcn_perm(P1, P1, 0x01010000u), pp3 = __builtin_amdgcn_perm(P1, P1, 0x03030202u);
        // row y: only the odd columns are new; gather them (cell i <-> byte i of P0/P1)
        u32 a0 = __builtin_amdgcn_perm(E.y, E.x, 0x07050301u), a1 = __builtin_amdgcn_perm(E.w, E.z, 0x07050301u);
        u32 q0 = quant4<IDENT>(a0, P0, slut), q1 = quant4<IDENT>(a1, P1, slut);
        uint4 o0 = make_uint4(__builtin_amdgcn_perm(q0, E.x, 0x05020400u), __builtin_amdgcn_perm(q0, E.y, 0x07020600u),
                              __builtin_amdgcn_perm(q1, E.z, 0x05020400u), __builtin_amdgcn_perm(q1, E.w, 0x07020600u));
        pitched_store16(out, dp, W, gx, gy, o0);
        __builtin_amdgcn_sched_barrier(0);   // row y + 1 after row y: this cold path must not set the kernel's register count
        if (gy + 1 < H) {
            uint4 o1 = make_uint4(quant4<IDENT>(O.x, pp0, slut), quant4<IDENT>(O.y, pp1, slut),
                                  quant4<IDENT>(O.z, pp2, slut), quant4<IDENT>(O.w, pp3, slut));
            pitched_store16(out, dp, W, gx, gy + 1, o1);
        }
    }
}
#endif

}  // namespace
}  // namespace hgi
