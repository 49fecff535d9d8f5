// Scaled decode (hgi_decode_scaled_u8_dev): every frame of a batch at 1 / 2^s resolution, i.e. the stride-2^s lattice of the full
// decode, decoded from the grid bytes of that lattice alone.
//
// A level pass writes only the points of its own lattice and never touches a coarser one again, so after levels - s passes the
// stride-2^s lattice is final; and it depends only on the grid bytes at the same lattice:
//     decode(grid, levels)[::2^s, ::2^s] == decode(grid[::2^s, ::2^s], max(levels - s, 0))
// The tile procedure of the fused decoder therefore runs unchanged -- staging into the same LDS layout, the cone / seeds,
// dec_tile_fast / dec_tile_edge -- on a STRIDED VIEW of the grid: an sw x sh frame, sw = ceil(W / 2^s), sh = ceil(H / 2^s), whose
// byte (x, y) is src[y * rp + (x << s)].  rp = W << s on the device (every 2^s-th row of the grid), rp = W on the host call's
// compact plane (the rows it uploaded).  One wave decodes one 128 x 64 tile of the OUTPUT lattice with levels - s levels.
//   * Staging.  Interior tiles read 16 view bytes per lane and row from 16 << s source bytes: s = 1 two 16-B loads and their even
//     bytes (even_bytes), s = 2 four and byte 0 of every dword, s >= 3 one byte load per view byte (every 128-B line of the
//     row is fetched at any of these steps up to 64, so the byte count is w * h / 2^s however they are picked).  The buffer range
//     check on the source frame supplies the out-of-image zeros below it; columns right of it are masked.  Ragged tiles and the
//     halo columns use byte loads: each is range-checked on its own.  A wide load may read past a row's last view byte -- into
//     the next row, never past the frame: tiles that would read the frame's last row that way are ragged (host side).
//   * Cone and seeds read the coarse lattice through the same view (cone_issue's `At` hook); deeper pyramids start from the
//     view's stride-256 lattice plane, gathered and decoded in front as decode_impl does.
//   * Stores: dec_tile_fast's 16-B row pairs for interior tiles, store_rows_edge's clipping at sw / sh for ragged ones, both
//     addressed through a descriptor of the output frame (any pitch, any alignment).
//   * Frames whose byte offsets do not fit 32 bits (and the knobs build's HGI_FORCE_CHECKED) take a byte-checked path.
#define HGI_FUSED_NO_LAUNCHERS 1
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"                 // the full decode's host geometry and byte-checked staging:
#pragma clang diagnostic ignored "-Wunneeded-internal-declaration"   // this unit has view forms of its own
#include "hgi_fused_dec.hip"   // the decode direction's build settings and tile procedure, 128 x 64 tiles
#pragma clang diagnostic pop

namespace hgi {
namespace {

// byte (x, y) of the view, relative to the source frame's first byte
struct ViewAt {
    u64 rp;
    u32 s;
    __device__ __forceinline__ size_t operator()(size_t x, size_t y, u32) const { return y * rp + (x << s); }
};

// The launch: the view's tile lattice.  The first ix x iy tiles of a frame are interior (body inside the view, buffer path
// allowed, wide loads safe); the others -- right of ix, then below iy -- are ragged and dispatched first, like block_role's.
struct Scaled {
    u32 sw, sh, s;
    u32 tx, ty, ix, iy;
    u32 ipf, epf, nf, nedge;
    FastDiv fd_ix, fd_ipf;
    u32 rp32, bytes32;           // buffer path: view row pitch and bytes of one source frame (num_records)
    u32 pitch, span;             // ... output pitch, bytes of one output frame (sh - 1) * pitch + sw
    u64 rp, istride;             // view row pitch, bytes between source frames
    u64 opitch, ostride;         // output pitch and bytes between output frames
};

__device__ __forceinline__ Tile scaled_tile(const Scaled &sc, bool &edge, bool &idle)
{
    const u32 b = blockIdx.x, ne8 = (sc.nedge + 7u) & ~7u;
    Tile tl;
    u32 tx, ty;
    edge = b < ne8;
    idle = edge && b >= sc.nedge;
    if (edge) {
        const u32 e = idle ? 0u : b;
        tl.frame = e / sc.epf;
        u32 i = e - tl.frame * sc.epf;
        const u32 right = (sc.tx - sc.ix) * sc.ty;
        if (i < right) {
            const u32 w = sc.tx - sc.ix;
            ty = i / w;
            tx = sc.ix + (i - ty * w);
        } else {
            i -= right;
            ty = sc.iy + i / sc.ix;
            tx = i % sc.ix;
        }
    } else {
        // interior tiles frame by frame, row-major, dealt to the XCDs in contiguous eighths (range_first)
        const u32 fb = b - ne8;
        const u32 t = range_first(sc.nf, fb & 7u) + (fb >> 3);
        tl.frame = fdiv(t, sc.fd_ipf);
        const u32 r = t - tl.frame * sc.ipf;
        ty = fdiv(r, sc.fd_ix);
        tx = r - ty * sc.ix;
    }
    tl.X0 = tx * TW;
    tl.Y0 = ty * TH;
    return tl;
}

// 16 view bytes of one row from source offset `off` (view byte j at off + (j << s)).  SH = 1 / 2: wide loads and a byte pick
// (s must equal SH); SH = 0: one range-checked byte load per view byte, any s.
template <int SH>
__device__ __forceinline__ v4u view16(__amdgpu_buffer_rsrc_t rs, u32 off, u32 s)
{
    v4u r;
    if (SH == 1) {
        const v4u a = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0), b = __builtin_amdgcn_raw_buffer_load_b128(rs, off + 16, 0, 0);
        const v2u ea = even_bytes(a), eb = even_bytes(b);
        r = v4u{ea.x, ea.y, eb.x, eb.y};
    } else if (SH == 2) {
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const v4u a = __builtin_amdgcn_raw_buffer_load_b128(rs, off + 16 * d, 0, 0);
            r[d] = __builtin_amdgcn_perm(a.y, a.x, 0x0c0c0400u) | __builtin_amdgcn_perm(a.w, a.z, 0x04000c0cu);
        }
    } else {
        u32 w[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 16; ++j) w[j >> 2] |= (u32)__builtin_amdgcn_raw_buffer_load_b8(rs, off + ((u32)j << s), 0, 0) << (8 * (j & 3));
        r = v4u{w[0], w[1], w[2], w[3]};
    }
    return r;
}

// stage_issue's loads on the view: even rows and halo rows (Stage.e, Stage.hv), the halo columns (Stage.x0 / d16 / d32 / d64,
// one byte load each), and -- ODD -- the odd rows in the fine-level lane map (Stage.o).  `vb` = the source offset of the
// tile's origin, Y0 * rp + (X0 << s).  RAGGED: chunks that start right of the view are not loaded, the one that straddles
// its right edge is masked; rows below it read 0 from the range check (source offset >= the frame's bytes).
template <int SH, bool RAGGED>
__device__ __forceinline__ void scaled_issue_rows(Stage &st, __amdgpu_buffer_rsrc_t rs, u32 vb, const Scaled &sc, Tile tl, int k, int nh)
{
    const int lane = HGI_LANE, c = lane & (CH - 1), r = lane >> LCH;
    const u32 rp = __builtin_amdgcn_readfirstlane(sc.rp32), s = __builtin_amdgcn_readfirstlane(sc.s), W = sc.sw;
    const u32 col = (16u * c) << s;
    const bool cin = !RAGGED || tl.X0 + 16 * c < W;
    const bool narrow = RAGGED && tl.X0 + TW > W;
    const v4u cm = narrow ? chunk_mask((int)W - (int)(tl.X0 + 16 * c)) : v4u{~0u, ~0u, ~0u, ~0u};
#pragma unroll
    for (int j = 0; j < TH / 16; ++j) {
        st.e[j] = v4u{0, 0, 0, 0};
        if (cin) st.e[j] = view16<SH>(rs, vb + (u32)(2 * (r + 8 * j)) * rp + col, s);
        if (narrow) st.e[j] &= cm;
    }
    st.hv = v4u{0, 0, 0, 0};
    if (lane < nh * CH && cin) st.hv = view16<SH>(rs, vb + (u32)(TH + hoff(r)) * rp + col, s);
    if (narrow) st.hv &= cm;
    const int hy = lane < TH / 2 ? 2 * lane : TH + hoff(lane - TH / 2);
    const u32 xo = vb + (u32)hy * rp, xr = tl.X0 + TW;      // first view column right of the tile
    u32 v[HR] = {0, 0, 0, 0, 0, 0};
    if (lane < TH / 2 + nh) {
        // column offset `off` is only ever touched on rows = 0 (mod off) (stage_issue)
#pragma unroll
        for (int i = 0; i < HR; ++i) {
            const u32 off = (u32)hoff(i);
            const bool want = i < 3 || ((int)k > i && !(hy & (int)(off - 1)));
            if (want && xr + off < W) v[i] = __builtin_amdgcn_raw_buffer_load_b8(rs, xo + ((TW + off) << s), 0, 0);
        }
    }
    st.x0 = v3u{v[0], v[1], v[2]};
    st.d16 = v[3];
    st.d32 = v[4];
    st.d64 = v[5];
    st.zero4 = st.zero8 = false;
}

template <int SH, bool RAGGED>
__device__ __forceinline__ void scaled_issue_odd(Stage &st, __amdgpu_buffer_rsrc_t rs, u32 vb, const Scaled &sc, Tile tl)
{
    const int c = HGI_LANE & (CH - 1);
    const u32 rp = __builtin_amdgcn_readfirstlane(sc.rp32), s = __builtin_amdgcn_readfirstlane(sc.s), W = sc.sw;
    const u32 vodd = vb + (u32)(2 * fine_pair0() + 1) * rp + ((16u * c) << s);
    const bool cin = !RAGGED || tl.X0 + 16 * c < W;
    const bool narrow = RAGGED && tl.X0 + TW > W;
    const v4u cm = narrow ? chunk_mask((int)W - (int)(tl.X0 + 16 * c)) : v4u{~0u, ~0u, ~0u, ~0u};
#pragma unroll
    for (int j = 0; j < NFINE; ++j) {
        st.o[j] = v4u{0, 0, 0, 0};
        if (cin) st.o[j] = view16<SH>(rs, vodd + (u32)(16 * j) * rp, s);
        if (narrow) st.o[j] &= cm;
    }
}

// ---- byte-checked path: 64-bit addressing, every view byte tested against the view ----------------------------------------
__device__ __forceinline__ u32 view_byte(const u8 *__restrict__ fr, const ViewAt &at, u32 W, u32 H, u32 x, u32 y)
{
    return (x < W && y < H) ? (u32)fr[at(x, y, W)] : 0u;
}

__device__ __forceinline__ uint4 view_load16(const u8 *__restrict__ fr, const ViewAt &at, u32 W, u32 H, u32 gx, u32 gy)
{
    u32 w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 16; ++j) w[j >> 2] |= view_byte(fr, at, W, H, gx + j, gy) << (8 * (j & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// stage_tile_generic on the view (the view by value: a reference to a kernel argument would be a copy on the stack)
__device__ __noinline__ void stage_scaled_generic(u8 *buf, const u8 *__restrict__ fr, u64 rp, u32 s, u32 W, u32 H, Tile tl, int nh)
{
    const ViewAt at = {rp, s};
    const int lane = HGI_LANE;
    for (int i = lane; i < (TH / 2 + nh) * CH; i += NL) {
        const int rr = i >> LCH, c = i & (CH - 1);
        const int y = rr < TH / 2 ? 2 * rr : TH + hoff(rr - TH / 2);
        *reinterpret_cast<uint4 *>(buf + rr * S + 16 * c) = view_load16(fr, at, W, H, tl.X0 + 16 * c, tl.Y0 + y);
    }
    for (int i = lane; i < 8 * (TH / 2 + nh); i += NL) {
        const int hc = i & 7, rr = i >> 3;
        if (hc >= nh) continue;
        const int off = hoff(hc);
        const int y = rr < TH / 2 ? 2 * rr : TH + hoff(rr - TH / 2);
        if (rr < TH / 2 && (y & ((off ? off : 2) - 1))) continue;
        buf[HCOL + hc * HP + rr] = (u8)view_byte(fr, at, W, H, tl.X0 + TW + off, tl.Y0 + y);
    }
}

// dec_fine_generic's arithmetic; odd rows from the view, byte stores into the pitched output frame, clipped to sw x sh
template <int INTERP>
__device__ __forceinline__ void dec_fine_generic_scaled(const u8 *buf, const u8 *__restrict__ fr, u8 *__restrict__ out, Tile tl, u32 W,
                                                     u32 H, u64 rp, u32 s, u64 opitch)
{
    const ViewAt at = {rp, s};
    for (int i = HGI_LANE; i < (TH / 2) * CH; i += NL) {
        const int z = i >> LCH, y = 2 * z, x = 16 * (i & (CH - 1));
        const u32 gx = tl.X0 + x, gy = tl.Y0 + y;
        if (gx >= W || gy >= H) continue;
        const u8 *r0 = buf + z * S + x;
        uint4 E = *reinterpret_cast<const uint4 *>(r0);
        uint4 O = view_load16(fr, at, W, H, gx, gy + 1);
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
        u8 *row0 = out + (size_t)gy * opitch + gx;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if (gx + j >= W) continue;
            row0[j] = (u8)(o0[j >> 2] >> (8 * (j & 3)));
            if (gy + 1 < H) row0[opitch + j] = (u8)(o1[j >> 2] >> (8 * (j & 3)));
        }
    }
}

// One block (= one wave) per tile of the view, ONE launch per batch.  SEEDED: 0 = the pyramid fits the tile; 2 = the cone
// (k == 4, sd.up levels above the tile; deeper pyramids on the view's stride-256 lattice planes).  SH: the interior tiles'
// loads (1, 2: wide loads for s = 1, 2; 0: byte loads).
// (s >= 2 keeps up to four times the full decode's load registers in flight: half its wave budget, no spills)
template <int INTERP, int SEEDED, int SH>
__global__ __launch_bounds__(NL) __attribute__((amdgpu_waves_per_eu(SH != 1 ? HGI_DEC_WAVES_PER_EU / 2 : SEEDED == 2 ? HGI_DEC_WAVES_PER_EU - 2 : HGI_DEC_WAVES_PER_EU))) void k_dec_scaled(
    const u8 *__restrict__ src, u8 *__restrict__ dst, u32 k, Seeds sd, Scaled sc, u32 fast)
{
    extern __shared__ __attribute__((aligned(16))) u8 smem[];
    const int nh = k >= 2 ? (int)k : 1;
    u8 *buf = smem - HCOL;
    const u32 W = sc.sw, H = sc.sh;
    bool edge, idle;
    const Tile tl = scaled_tile(sc, edge, idle);
    if (idle) return;
    const u8 *fr = src + (size_t)tl.frame * sc.istride;
    u8 *out = dst + (size_t)tl.frame * sc.ostride;
    const ViewAt at = {sc.rp, sc.s};
    SeedRegs seeds;
    ConeLane cone;
    if (fast) {   // 32-bit buffer offsets on both sides
        Buf bo;   // the store side: the output frame
        bo.rs = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(fr), 0, sc.bytes32, 0x00020000);
        bo.rd = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(out), 0, sc.span, 0x00020000);
        bo.W = sc.pitch;
        bo.base = __builtin_amdgcn_readfirstlane(tl.Y0 * sc.pitch + tl.X0);
        const u32 vb = __builtin_amdgcn_readfirstlane(tl.Y0 * sc.rp32 + (tl.X0 << sc.s));
        Stage st;
        if (!edge) {
            scaled_issue_rows<SH, false>(st, bo.rs, vb, sc, tl, (int)k, nh);
            if (SEEDED == 2) cone = cone_issue<false>(fr, W, H, sd, tl, at);
            stage_commit<false>(buf, nullptr, st, nh);
            LDS_ORDER();
            scaled_issue_odd<SH, false>(st, bo.rs, vb, sc, tl);      // in flight while the coarse levels run (HGI_ODD_LATE)
        } else {
            if (SEEDED == 2) cone = cone_issue<false>(fr, W, H, sd, tl, at);
            scaled_issue_rows<0, true>(st, bo.rs, vb, sc, tl, (int)k, nh);
            scaled_issue_odd<0, true>(st, bo.rs, vb, sc, tl);
            stage_commit<false>(buf, nullptr, st, nh);
            LDS_ORDER();
        }
        if (SEEDED == 2) seeds = cone_finish<INTERP, false, true>(cone, buf, nullptr, sd.up, nullptr);
        LDS_ORDER();
        if (SEEDED) dec_seed_commit(buf, seeds, k);
        if (edge)
            dec_tile_edge<INTERP, 2>(buf, TileCtx{tl, bo}, st.o, k, W, H);
        else
            dec_tile_fast<INTERP>(buf, TileCtx{tl, bo}, st.o, k, W, H);
        return;
    }
    // views whose byte offsets (or outputs whose span) do not fit 32 bits: every access checked, 64-bit addressing
    if (SEEDED == 2) cone = cone_issue<false>(fr, W, H, sd, tl, at);
    stage_scaled_generic(buf, fr, sc.rp, sc.s, W, H, tl, nh);
    LDS_ORDER();
    if (SEEDED == 2) seeds = cone_finish<INTERP, false, true>(cone, buf, nullptr, sd.up, nullptr);
    if (SEEDED) dec_seed_commit(buf, seeds, k);
    for (int s = 1 << (k - 1); s >= 2; s >>= 1) {
        dec_cells<INTERP, true>(buf, s, tl, W, H);
        dec_halo_cells<INTERP>(buf, s, tl, W, H);
        LDS_ORDER();
    }
    dec_fine_generic_scaled<INTERP>(buf, fr, out, tl, W, H, sc.rp, sc.s, sc.opitch);
}

// dst[f][y * dst_pitch + x] = src[f][(y << ky) * rp + (x << kx)]: a lattice of the view as a pitched plane
__global__ void k_gather_view(const u8 *__restrict__ src, u64 src_stride, u64 rp, u32 ky, u32 kx, u32 sw, u32 sh, u8 *__restrict__ dst,
                              u64 dst_pitch, u64 dst_stride, u32 batch)
{
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (u64)sw * sh) return;
    const u64 y = i / sw, x = i - y * sw;
    for (u32 f = blockIdx.y; f < batch; f += gridDim.y)
        dst[f * dst_stride + y * dst_pitch + x] = src[f * src_stride + (y << ky) * rp + (x << kx)];
}

}  // namespace

hipError_t launch_gather_view(const uint8_t *src, uint64_t src_stride, uint64_t row_pitch, uint32_t ky, uint32_t kx, uint32_t sw,
                              uint32_t sh, uint8_t *dst, uint64_t dst_pitch, uint64_t dst_stride, uint32_t batch, hipStream_t s)
{
    const u64 n = (u64)sw * sh, blocks = (n + 255) / 256;
    if (n == 0 || batch == 0) return hipSuccess;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_gather_view, dim3((u32)blocks, batch < 65535u ? batch : 65535u), dim3(256), 0, s, src, src_stride, row_pitch,
                       ky, kx, sw, sh, dst, dst_pitch, dst_stride, batch);
    return hipGetLastError();
}

hipError_t launch_decode_scaled(const uint8_t *src, uint8_t *out, const ScaledView &v, uint32_t k, int interp, const Seeds *seeds,
                                hipStream_t s)
{
    if (k < 1 || k > (u32)MAXK || v.width == 0 || v.height == 0 || v.batch == 0 || v.shift > 31) return hipErrorInvalidValue;
    if (seeds && k < (uint32_t)kSeededMinLevels) return hipErrorInvalidValue;
    const bool cone = seeds && seeds->up != 0;
    if (seeds && (!cone || k != 4 || seeds->up > (u32)kConeMaxUp)) return hipErrorInvalidValue;   // (no seed-plane route here)
    Scaled sc;
    sc.sw = v.width;
    sc.sh = v.height;
    sc.s = v.shift;
    sc.rp = v.row_pitch;
    sc.istride = v.frame_stride;
    sc.opitch = v.out_pitch;
    sc.ostride = v.out_frame_stride;
    sc.tx = (v.width + TW - 1) / TW;
    sc.ty = (v.height + TH - 1) / TH;
    const int nh = k >= 2 ? (int)k : 1;
    // the read side: every 32-bit buffer offset the staging forms -- rows up to the last tile's halo (TH + 64 below its origin),
    // columns up to its halo columns (TW + 64) plus a chunk's 16 << s bytes
    const u64 rows_max = (u64)sc.ty * TH + 64, cols_max = ((u64)sc.tx * TW + 64 + 16) << v.shift;
    const bool read32 = v.shift < 32 && rows_max * v.row_pitch + cols_max + 64 < (1ull << 32) && v.frame_bytes < (1ull << 32);
    const StoreSide st = store_side_32(v.height, v.width, v.out_pitch);      // one output frame addressed with 32 bits
    const bool fast = read32 && st.ok && !HGI_SWITCH(HGI_FORCE_CHECKED);
    sc.rp32 = fast ? (u32)v.row_pitch : 0u;
    sc.bytes32 = fast ? (u32)v.frame_bytes : 0u;
    sc.pitch = fast ? (u32)st.pitch : 0u;
    sc.span = fast ? (u32)st.span : 0u;
    sc.ix = fast ? v.width / TW : 0u;
    sc.iy = fast ? v.height / TH : 0u;
    // A wide load reads 16 << s bytes for a chunk's 16 view bytes: on the frame's last source row the dword after the row's last
    // view byte can lie past the frame's end, and the range check would drop it whole.  Interior tiles then keep off that row
    // (the view row sh - 1, which a tile reads up to TH + hoff(nh - 1) rows below its origin).
    const u32 reach = TH + (nh >= 2 ? (2u << (nh - 1)) : 0u);
    const bool hazard = (u64)(v.height - 1) * v.row_pitch + (((u64)sc.ix * TW) << v.shift) > v.frame_bytes;
    if (hazard)
        while (sc.iy > 0 && (u64)(sc.iy - 1) * TH + reach >= v.height - 1) --sc.iy;
    if (sc.ix == 0 || sc.iy == 0) sc.ix = sc.iy = 0;
    sc.ipf = sc.ix * sc.iy;
    sc.epf = sc.tx * sc.ty - sc.ipf;
    const u64 nf = (u64)sc.ipf * v.batch, ne = (u64)sc.epf * v.batch;
    if (nf + ne + 8 >= (1ull << 31)) return hipErrorInvalidValue;
    sc.nf = (u32)nf;
    sc.nedge = (u32)ne;
    sc.fd_ix = make_fastdiv(sc.ix ? sc.ix : 1u);
    sc.fd_ipf = make_fastdiv(sc.ipf ? sc.ipf : 1u);
    Seeds sd = seeds ? *seeds : Seeds{nullptr, nullptr, 0, 0, 0, 0};
    const size_t lds = lds_for_waves((size_t)buf_bytes(nh), dec_resident_tiles(nf + ne, v.width, k, seeds != nullptr));
    const dim3 blocks(((sc.nedge + 7u) & ~7u) + sc.nf);
    const u32 fastu = fast ? 1u : 0u;
    return with_choices(
        [&](auto I, auto SE, auto SH) { return launch_tile_kernel<k_dec_scaled<I, SE, SH>>(blocks, lds, s, src, out, k, sd, sc, fastu); },
        interp_choice(interp), OneOf<2, 0>{cone ? 2 : 0}, OneOf<1, 2, 0>{v.shift == 1 ? 1 : v.shift == 2 ? 2 : 0});
}

}  // namespace hgi
