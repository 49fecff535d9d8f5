// Typed encode (hgi_typed_encode_dev): frames of float16 / bfloat16 / float32 elements to grids in one launch.  Each tile runs
// k_enc_pitched's fast path (csrc/hgi_fused_pitched_enc.hip) as it stands -- the block -> tile map, the table in LDS,
// stage_commit, the cone's walk, the coarse-level chain, level 2, the finest pass and its stores -- behind a staging of its own:
// typed_issue / typed_issue_odd / cone_issue_typed load E-byte elements where pitched_issue / pitched_issue_odd / cone_issue
// load bytes, convert them (include/hgi_typed.h: two separately rounded float32 operations, round half to even, clamp, NaN ->
// 0) and leave in Stage and ConeLane the packed pixel bytes those functions would have loaded from the converted image.
//
// Zero means pixel 0.  The byte encoder takes "outside the image" from the descriptor's range check, which returns the byte 0.
// Here the same check returns the ELEMENT 0.0, whose pixel is clamp(rint(bias)): so every load outside the image is predicated
// off and its pixels are set to 0 AFTER conversion -- rows at and below the height, chunks and halo columns right of the width,
// the cone's points outside the plane -- and the byte masks of a ragged chunk are applied to converted pixels, as before.  Gap
// bytes right of a row's end are converted with the chunk that straddles the edge (any bit pattern converts: no operation
// here traps) and masked out.
//
// Registers.  16 pixels are 4 dwords packed and 4 * E dwords as loaded, so the loads are issued, converted and packed in
// batches of typed_batch(E) row groups, 32 dwords as loaded whatever E is: the even rows of an interior tile in one (E = 2) or
// two (E = 4) batches; the odd rows likewise, the first batch in flight while the even rows are committed to LDS, the second
// (E = 4) behind it, all converted BEFORE the coarse levels -- the byte encoder holds its 16 odd-row dwords across them; 64
// unconverted ones cannot wait there.  The kernels are compiled for kTypedWavesPerEu waves per SIMD;
// tests/test_typed.py holds the ISA to it.
//
// Load layout: each lane loads the 16 * E contiguous bytes of its own 16 pixels, E b128 loads, lanes 16 * E bytes apart.  Measured
// with this layout (profiles/r13_typed.txt): 1.19x - 1.58x the copy of the launch's own bytes.  The line-filling alternative (an
// exchange through LDS, as mapped decode's stores make) is not built: DESIGN.md 4.12.
// This is the 64-row build of the encoder, buffer path only: hgi_typed.hip refuses the calls whose offsets need 64 bits.
#define HGI_FUSED_NO_LAUNCHERS 1
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"
#pragma clang diagnostic ignored "-Wunneeded-internal-declaration"
#include "../csrc/hgi_fused_enc.hip"   // the encode direction's build settings and tile procedure, 128 x 64 tiles
#include "../csrc/hgi_fused_pitched.h"
#pragma clang diagnostic pop
#include "../companion/hgi_tile.h"
#include "hgi_typed_kernels.h"

namespace hgi {
namespace {

// Row groups (16 pixels per lane each) whose elements are in flight together: 32 dwords as loaded, whatever E is.
__host__ __device__ constexpr int typed_batch(int elem) { return elem == 4 ? 2 : 4; }
static_assert(NFINE % typed_batch(4) == 0 && NFINE % typed_batch(2) == 0 && (TH / 16) % typed_batch(4) == 0 && (TH / 16) % typed_batch(2) == 0,
              "row groups come in whole batches");
// Waves per SIMD the kernels are compiled for (512 VGPRs per SIMD lane, allocated in eights): DESIGN.md 4.12
constexpr int kTypedWavesPerEu = HGI_ENC_WAVES_PER_EU;

// The conversion's launch constants.  bf: the 2-byte elements are bfloat16 (wave-uniform).
struct Cvt {
    float scale, bias;
    u32 bf;
};

// include/hgi_typed.h, the conversion: t = fl32(fl32(x * scale) + bias), two roundings (never contracted into an fma);
// v_rndne_f32 rounds half to even; v_cvt_u32_f32 gives 0 for NaN and for everything negative (-inf included) and saturates
// above, so one unsigned minimum finishes the clamp.  Denormals are kept (the kernels' float mode; checked in the ISA).
__device__ __forceinline__ float px_round(float x, const Cvt &cv)
{
#pragma clang fp contract(off)
    const float m = x * cv.scale;
    const float t = m + cv.bias;
    return __builtin_rintf(t);
}

__device__ __forceinline__ u32 px_of(float x, const Cvt &cv)
{
    u32 u;
    asm("v_cvt_u32_f32 %0, %1" : "=v"(u) : "v"(px_round(x, cv)));
    return u < 255u ? u : 255u;
}

// Four pixels -> one packed dword, in ONE statement: left to itself the compiler converts a whole batch first and packs it
// afterwards, one register per PIXEL in between, which is what the batches exist to avoid.  Plain VALU operations on whole
// registers (no SDWA, no DPP, no transcendental): no wait states are owed between them.
__device__ __forceinline__ u32 px_pack4(float x0, float x1, float x2, float x3, const Cvt &cv)
{
    const float r0 = px_round(x0, cv), r1 = px_round(x1, cv), r2 = px_round(x2, cv), r3 = px_round(x3, cv);
    u32 d, t;
    asm("v_cvt_u32_f32 %0, %2\n\t"
        "v_cvt_u32_f32 %1, %3\n\t"
        "v_min_u32 %0, 0xff, %0\n\t"
        "v_min_u32 %1, 0xff, %1\n\t"
        "v_lshl_or_b32 %0, %1, 8, %0\n\t"
        "v_cvt_u32_f32 %1, %4\n\t"
        "v_min_u32 %1, 0xff, %1\n\t"
        "v_lshl_or_b32 %0, %1, 16, %0\n\t"
        "v_cvt_u32_f32 %1, %5\n\t"
        "v_min_u32 %1, 0xff, %1\n\t"
        "v_lshl_or_b32 %0, %1, 24, %0"
        : "=&v"(d), "=&v"(t)
        : "v"(r0), "v"(r1), "v"(r2), "v"(r3));
    return d;
}

__device__ __forceinline__ float as_f32(u32 w) { return __builtin_bit_cast(float, w); }

// the two 2-byte elements of a dword, widened exactly
template <bool BF>
__device__ __forceinline__ float lo16(u32 w)
{
    if (BF) return as_f32(w << 16);
    return (float)__builtin_bit_cast(_Float16, (unsigned short)w);
}
template <bool BF>
__device__ __forceinline__ float hi16(u32 w)
{
    if (BF) return as_f32(w & 0xffff0000u);
    return (float)__builtin_bit_cast(_Float16, (unsigned short)(w >> 16));
}

// 16 pixels as loaded: E b128 registers (the lane's 16 * E contiguous bytes)
template <int E>
struct Raw16 {
    v4u r[E];
};

template <int E, int AUX>
__device__ __forceinline__ void load16e(Raw16<E> &q, __amdgpu_buffer_rsrc_t rs, u32 voff, u32 soff)
{
#pragma unroll
    for (int i = 0; i < E; ++i) q.r[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, voff + 16 * i, soff, AUX);
}

template <int E>
__device__ __forceinline__ void clear16(Raw16<E> &q)
{
#pragma unroll
    for (int i = 0; i < E; ++i) q.r[i] = v4u{0, 0, 0, 0};
}

template <int E, bool BF>
__device__ __forceinline__ v4u cvt16_as(const Raw16<E> &q, const Cvt &cv)
{
    v4u o;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        if (E == 4) {
            const u32 w0 = q.r[d].x, w1 = q.r[d].y, w2 = q.r[d].z, w3 = q.r[d].w;      // (values: a vector's element is no object to cast)
            o[d] = px_pack4(as_f32(w0), as_f32(w1), as_f32(w2), as_f32(w3), cv);
        } else {
            const u32 w0 = q.r[d >> 1][2 * (d & 1)], w1 = q.r[d >> 1][2 * (d & 1) + 1];
            o[d] = px_pack4(lo16<BF>(w0), hi16<BF>(w0), lo16<BF>(w1), hi16<BF>(w1), cv);
        }
    }
    return o;
}


// the packed pixels of 16 loaded elements.  The kind of a 2-byte element is a launch constant, tested per chunk: a branch
// around the whole staging instead lets the compiler hoist the loads of every batch in front of it, and the kernel spills.
template <int E>
__device__ __forceinline__ v4u cvt16(const Raw16<E> &q, const Cvt &cv)
{
    if (E == 2 && cv.bf) return cvt16_as<E, true>(q, cv);
    return cvt16_as<E, false>(q, cv);
}

// one element on its own (halo columns, cone points): the load and the pixel
template <int E>
__device__ __forceinline__ u32 load1(__amdgpu_buffer_rsrc_t rs, u32 voff)
{
    if (E == 4) return __builtin_amdgcn_raw_buffer_load_b32(rs, voff, 0, 0);
    return (u32)(unsigned short)__builtin_amdgcn_raw_buffer_load_b16(rs, voff, 0, 0);
}
template <int E>
__device__ __forceinline__ u32 px1(u32 w, const Cvt &cv)
{
    if (E == 4) return px_of(as_f32(w), cv);
    return px_of(cv.bf ? lo16<true>(w) : lo16<false>(w), cv);
}

// pitched_issue for E-byte elements: `rb` and `pitch` are bytes, every test against the image is in pixels.  Each load is
// predicated on its pixels lying inside the image and each result is 0 where the predicate fails (the header above).  RAGGED
// tiles load their odd rows here as well (pitched_issue<true, true>); interior tiles take them from typed_issue_odd.
template <int E, bool RAGGED>
__device__ __forceinline__ void typed_issue(Stage &st, __amdgpu_buffer_rsrc_t rs, u32 rb, u32 pitch, u32 W, u32 H, Tile tl, int k, int nh,
                                            const Cvt &cv)
{
    const int lane = HGI_LANE, c = lane & (CH - 1), r = lane >> LCH;
    const u32 P = __builtin_amdgcn_readfirstlane(pitch);   // soffset operands must be provably uniform
    const u32 voff = rb + 2 * r * P + 16 * E * c;                          // even rows 2 * (r + 8 j)
    const u32 vodd = rb + (2 * fine_pair0() + 1) * P + 16 * E * c;         // odd rows 2 * (pair0 + 8 it) + 1
    const bool cin = tl.X0 + 16 * c < W;
    const bool narrow = RAGGED && tl.X0 + TW > W;   // wave-uniform: this tile straddles the right edge
    const v4u cm = narrow ? chunk_mask((int)W - (int)(tl.X0 + 16 * c)) : v4u{~0u, ~0u, ~0u, ~0u};
    const v4u none = {0, 0, 0, 0};
    // halo columns: one lane per (even) row, single elements at offsets 0/4/8 and, on the rows that touch them, 16/32/64
    const int hy = lane < TH / 2 ? 2 * lane : TH + hoff(lane - TH / 2);
    const u32 xo = rb + hy * P + TW * E;
    const u32 xr = tl.X0 + TW;              // first column right of the tile
    const bool hrow = lane < TH / 2 + nh && tl.Y0 + hy < H;
    const bool h0 = hrow && xr < W, h4 = hrow && xr + 4 < W, h8 = hrow && xr + 8 < W;
    const bool h16 = hrow && k >= 4 && !(hy & 15) && xr + 16 < W, h32 = hrow && k >= 5 && !(hy & 31) && xr + 32 < W,
               h64 = hrow && k >= 6 && !(hy & 63) && xr + 64 < W;
    u32 w0 = 0, w4 = 0, w8 = 0, w16 = 0, w32 = 0, w64 = 0;
    if (h0) w0 = load1<E>(rs, xo);
    if (h4) w4 = load1<E>(rs, xo + 4 * E);
    if (h8) w8 = load1<E>(rs, xo + 8 * E);
    if (h16) w16 = load1<E>(rs, xo + 16 * E);
    if (h32) w32 = load1<E>(rs, xo + 32 * E);
    if (h64) w64 = load1<E>(rs, xo + 64 * E);
    // halo rows TH + {0,4,8,..}: full lines
    const bool hvin = lane < nh * CH && cin && tl.Y0 + TH + hoff(r) < H;
    Raw16<E> qh;
    clear16(qh);
    if (hvin) load16e<E, 0>(qh, rs, rb + (TH + hoff(r)) * P + 16 * E * c, 0);
    // even rows, typed_batch(E) row groups in flight at a time; the halo's loads, issued in front, are converted behind the
    // first batch
    constexpr int NB = typed_batch(E);
#pragma unroll
    for (int j0 = 0; j0 < TH / 16; j0 += NB) {
        Raw16<E> q[NB];
        bool in[NB];
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int j = j0 + i;
            in[i] = !RAGGED || (cin && tl.Y0 + 2 * (r + 8 * j) < H);
            if (RAGGED) {      // chunks right of the width are not fetched; rows below the image are (the descriptor bounds them)
                clear16(q[i]);
                if (cin) load16e<E, 0>(q[i], rs, voff + j * 16 * P, 0);
            } else {
                load16e<E, HGI_LOAD_AUX>(q[i], rs, voff, j * 16 * P);
            }
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const v4u v = cvt16<E>(q[i], cv);
            st.e[j0 + i] = in[i] ? v & cm : none;
        }
        if (j0 == 0) {
            const v4u vh = cvt16<E>(qh, cv);
            st.hv = hvin ? vh & cm : none;
            st.x0 = v3u{h0 ? px1<E>(w0, cv) : 0u, h4 ? px1<E>(w4, cv) : 0u, h8 ? px1<E>(w8, cv) : 0u};
            st.d16 = h16 ? px1<E>(w16, cv) : 0u;
            st.d32 = h32 ? px1<E>(w32, cv) : 0u;
            st.d64 = h64 ? px1<E>(w64, cv) : 0u;
        }
        __builtin_amdgcn_sched_barrier(0);   // the next batch's registers are this batch's
    }
    st.zero4 = xr + 4 >= W;     // as pitched_issue leaves them (the bytes they clear at commit are 0 already)
    st.zero8 = xr + 8 >= W;
#pragma unroll
    for (int j0 = 0; j0 < NFINE; j0 += NB) {
        if (RAGGED) {
            Raw16<E> q[NB];
            bool in[NB];
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const int j = j0 + i;
                in[i] = cin && tl.Y0 + 2 * (fine_pair0() + 8 * j) + 1 < H;
                clear16(q[i]);
                if (cin) load16e<E, HGI_ODD_LOAD_AUX>(q[i], rs, vodd + j * 16 * P, 0);
            }
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const v4u v = cvt16<E>(q[i], cv);
                st.o[j0 + i] = in[i] ? v & cm : none;
            }
            __builtin_amdgcn_sched_barrier(0);
        } else {
#pragma unroll
            for (int i = 0; i < NB; ++i) st.o[j0 + i] = none;
        }
    }
}

// The odd rows of an interior tile as loaded (pitched_issue_odd), typed_batch(E) row groups from j0 on: the first batch is
// requested before the even rows are committed and converted behind the commit, the second (E = 4) is requested then and
// converted behind the cone's walk -- none waits unconverted across the coarse levels.
template <int E>
struct RawOdd {
    Raw16<E> q[typed_batch(E)];
};

template <int E>
__device__ __forceinline__ void typed_issue_odd(RawOdd<E> &ro, __amdgpu_buffer_rsrc_t rs, u32 rb, u32 pitch, int j0)
{
    const int c = HGI_LANE & (CH - 1);
    const u32 P = __builtin_amdgcn_readfirstlane(pitch);
    const u32 vodd = rb + (2 * fine_pair0() + 1) * P + 16 * E * c;
#pragma unroll
    for (int i = 0; i < typed_batch(E); ++i) load16e<E, HGI_ODD_LOAD_AUX>(ro.q[i], rs, vodd, (j0 + i) * 16 * P);
}

template <int E>
__device__ __forceinline__ void typed_convert_odd(Stage &st, const RawOdd<E> &ro, const Cvt &cv, int j0)
{
#pragma unroll
    for (int i = 0; i < typed_batch(E); ++i) st.o[j0 + i] = cvt16<E>(ro.q[i], cv);
}

// cone_issue for E-byte elements, of a frame that supplies its own base samples (no seed planes: hgi_typed.hip serves up to
// eight levels): the same index work, and the one load -- of an element, through the image's descriptor -- whose raw bits wait
// in ConeLane::v until cone_convert_typed.
template <int E>
__device__ __forceinline__ ConeLane cone_issue_typed(__amdgpu_buffer_rsrc_t rs, u32 pitch, u32 W, u32 H, const Seeds &sd, Tile tl)
{
    const u32 up = sd.up, sw = ((W - 1u) >> 4) + 1u, sh = ((H - 1u) >> 4) + 1u;      // the stride-16 plane
    constexpr u32 o2 = cone_off(2), o3 = cone_off(3), o4 = cone_off(4), o5 = cone_off(5);
    constexpr u32 nx0 = cone_n(TW, 0), ny0 = cone_n(TH, 0);
    const u32 lane = HGI_LANE, A = tl.X0 >> 4, B = tl.Y0 >> 4;
    ConeLane c;
    // levels 1 .. 4
    const u32 t = 1u + (lane >= o2) + (lane >= o3) + (lane >= o4);
    const u32 first = t == 1 ? 0u : t == 2 ? o2 : t == 3 ? o3 : o4;
    const u32 nx = t == 1 ? (u32)cone_n(TW, 1) : t == 2 ? (u32)cone_n(TW, 2) : t == 3 ? (u32)cone_n(TW, 3) : (u32)cone_n(TW, 4);
    const u32 rcp = t == 1 ? 43u : t == 2 ? 64u : 86u;      // (i * rcp) >> 8 == i / nx for nx = 6, 4, 3 and i < 64
    static_assert(cone_n(TW, 1) == 6 && cone_n(TW, 2) == 4 && cone_n(TW, 3) == 3 && cone_n(TW, 4) == 3, "reciprocals above");
    const u32 i = lane - first, iy = (i * rcp) >> 8, ix = i - iy * nx, m = (1u << t) - 1u;
    const u32 x = (A & ~m) + (ix << t), y = (B & ~m) + (iy << t);
    const bool on = lane < o5 && t <= up;
    c.t = on ? t : 0u;
    c.in1 = on && x < sw && y < sh;
    c.down1 = !((x | y) & (1u << t));
    c.nx1 = t == 1 ? (u32)cone_n(TW, 2) : (u32)cone_n(TW, 3);      // (level 4 has no coarser array)
    c.from1 = (t == 1 ? o2 : t == 2 ? o3 : o4) + cone_corner(x, y, A, B, t, c.nx1);
    const bool framed = x >= A && x < A + nx0 && y >= B && y < B + ny0;
    c.framed1 = c.in1 && framed;
    c.src1 = c.framed1 ? (u32)laddr((int)((x - A) << 4), (int)((y - B) << 4)) : 0u;
    c.v = c.vq = 0u;
    if (c.in1 && !framed) c.v = load1<E>(rs, (y << 4) * pitch + (x << 4) * E);      // inside the image: below the records
    // level 0: the seeds
    const u32 by = (lane * 26u) >> 8, bx = lane - by * nx0;      // lane / 10
    static_assert(nx0 == 10, "reciprocal above");
    c.on0 = lane < nx0 * ny0;
    c.in0 = c.on0 && A + bx < sw && B + by < sh;
    c.down0 = !(((A + bx) | (B + by)) & 1u);      // (B is odd for every other row of 16-row tiles)
    c.from0 = cone_corner(A + bx, B + by, A, B, 0u, (u32)cone_n(TW, 1));
    c.src0 = c.on0 ? (u32)laddr((int)(bx << 4), (int)(by << 4)) : 0u;
    return c;
}

// The loaded element becomes its pixel; a lane that loaded nothing keeps the pixel 0.  Base samples of the frame itself:
// residual == sample (cone_issue).
template <int E>
__device__ __forceinline__ void cone_convert_typed(ConeLane &c, const Cvt &cv)
{
    const u32 v = px1<E>(c.v, cv);
    c.v = c.vq = c.in1 && !c.framed1 ? v : 0u;
}

// SEEDED: 0 the tile holds the pyramid, 2 the cone on the frame's own samples (k == 4).  E: bytes per element.
template <int INTERP, bool IDENT, int SEEDED, int E>
__global__ __launch_bounds__(NL) __attribute__((amdgpu_waves_per_eu(kTypedWavesPerEu))) void k_enc_typed(
    const u8 *__restrict__ src, u8 *__restrict__ dst, u32 k, Lut256 lut, Seeds sd, TypedPlan tp, Cvt cv)
{
    extern __shared__ __attribute__((aligned(16))) u8 smem[];
    const PitchedPlan &p = tp.p;
    const int nh = k >= 2 ? (int)k : 1;
    // the table at LDS offset 0 (lut_at(); launch_encode_typed checks on the host that there is no static LDS)
    u8 *slut = smem;
    u8 *buf = smem + 256 - HCOL;
    u8 *rbuf = smem + 256 + buf_bytes(nh) - RCOL;
    const u32 W = p.W, H = p.H;
    bool edge, idle;
    const Tile tl = pitched_block_tile(p, edge, idle);
    if (idle) return;
    const u8 *fr = src + (size_t)tl.frame * tp.x.stride;
    u8 *out = dst + (size_t)tl.frame * p.dstride;
    SeedRegs seeds;
    ConeLane cone;
    // 32-bit buffer offsets on both sides (the host launches nothing else): bytes on the image side, pixels on the grid's
    TileCtx cur;
    cur.tl = tl;
    cur.b.rs = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(fr), 0, tp.x.rec, 0x00020000);
    cur.b.rd = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(out), 0, p.drec, 0x00020000);
    cur.b.W = p.dp32;
    cur.b.base = __builtin_amdgcn_readfirstlane(tl.Y0 * p.dp32 + tl.X0);
    const u32 rb = __builtin_amdgcn_readfirstlane(tl.Y0 * tp.x.pitch32 + tl.X0 * E);
    Stage st;
    u32 lutv = 0;
    if (!edge) {
        constexpr int NB = typed_batch(E);
        RawOdd<E> ro;
        typed_issue<E, false>(st, cur.b.rs, rb, tp.x.pitch32, W, H, tl, (int)k, nh, cv);
        typed_issue_odd<E>(ro, cur.b.rs, rb, tp.x.pitch32, 0);
        if (SEEDED == 2) cone = cone_issue_typed<E>(cur.b.rs, tp.x.pitch32, W, H, sd, tl);
        if (!IDENT) lutv = lut.w[HGI_LANE];
        stage_commit<true>(buf, rbuf, st, nh);
        if (!IDENT) reinterpret_cast<u32 *>(slut)[HGI_LANE] = lutv;
        LDS_ORDER();
        typed_convert_odd<E>(st, ro, cv, 0);
        if (NB < NFINE) {
            __builtin_amdgcn_sched_barrier(0);
            typed_issue_odd<E>(ro, cur.b.rs, rb, tp.x.pitch32, NB);
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
    if (SEEDED == 2) cone = cone_issue_typed<E>(cur.b.rs, tp.x.pitch32, W, H, sd, tl);
    typed_issue<E, true>(st, cur.b.rs, rb, tp.x.pitch32, W, H, tl, (int)k, nh, cv);
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

hipError_t launch_encode_typed(const void *img, uint8_t *grid, const TypedPlan &tp, uint32_t elem, bool bf16, float scale, float bias,
                               uint32_t k, uint32_t up, int interp, const Lut256 &lut, bool ident, hipStream_t s)
{
    const TileLaunch t = tile_launch(tp.p, k, up);
    if (!t.ok || (elem != 2 && elem != 4) || (bf16 && elem != 2)) return hipErrorInvalidValue;
    const Cvt cv = {scale, bias, bf16 ? 1u : 0u};
    const u8 *src = static_cast<const u8 *>(img);
    return with_choices(
        [&](auto I, auto ID, auto SE, auto EL) {
            return launch_tile_kernel<k_enc_typed<I, ID != 0, SE, EL>>(t.blocks, enc_lds_bytes(t.nh), s, src, grid, k, lut, t.sd, tp, cv);
        },
        interp_choice(interp), OneOf<1, 0>{ident ? 1 : 0}, OneOf<2, 0>{t.cone ? 2 : 0}, OneOf<4, 2>{(int)elem});
}

}  // namespace hgi
