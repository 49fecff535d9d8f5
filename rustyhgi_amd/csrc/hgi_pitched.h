// Pitched frames (hgi_encode_u8_pitched_dev / hgi_decode_u8_pitched_dev): frames whose rows lie `pitch` >= width bytes apart,
// with a pitch of its own on the read and on the write side.  The host plan -- which tiles are interior, whether the buffer
// path's 32-bit offsets hold, the descriptors' sizes -- and the block -> tile map the pitched kernels run
// (hgi_fused_pitched_dec.hip, hgi_fused_pitched_enc.hip).  Plain C++: tests/cpp/test_pitched_plan.cpp runs it with g++.
//
// A frame's SPAN is (height - 1) * pitch + width bytes: its first byte to its last.  Row y >= height starts at y * pitch >=
// the span, so a buffer descriptor of `span` records returns 0 for it (the out-of-image rule below the image) and drops a
// store to it; columns right of `width` are inside the span on every row but the last and are handled by masks.
//
// Launch order: the ragged tiles of all frames first (right column, then bottom rows; their count padded to a
// multiple of eight), then the interior tiles frame by frame, row-major, dealt to the eight XCDs in contiguous eighths.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "hgi_fastdiv.h"

namespace hgi {

constexpr uint32_t kPitchedTileW = 128, kPitchedTileH = 64;   // the 64-row build of both directions

struct PitchedFrames {
    uint32_t width, height, batch;
    uint64_t src_pitch, dst_pitch;            // bytes between rows
    uint64_t src_stride, dst_stride;          // bytes between frames
};

// What a pitched launch reads (kernel argument, by value).
struct PitchedPlan {
    uint32_t W, H;
    uint32_t tx, ty, ix, iy;                  // all tiles of a frame; tiles whose body lies inside the image (0 x 0: none)
    uint32_t ipf, epf, nf, nedge;             // interior / ragged tiles per frame and over the batch
    FastDiv fd_ix, fd_ipf;
    uint32_t fast;                            // 1: buffer path (32-bit offsets on both sides); 0: byte-checked, 64-bit addressing
    uint32_t sp32, dp32;                      // buffer path: read and write pitch
    uint32_t srec, drec;                      // ... num_records of the read (span + tail) and write (span) descriptors
    uint64_t sp, dp, sstride, dstride;
    bool ok;                                  // host only: the launch fits (tile count)
};

// Bytes from a frame's first byte to its last.  A one-row frame never steps by its pitch.
HGI_HD inline uint64_t pitched_span(uint32_t w, uint32_t h, uint64_t pitch) { return (uint64_t)(h - 1) * pitch + w; }

// src: address of the first INPUT frame.  Rows that are not a multiple of 4 bytes: the dword that holds a row's last bytes
// straddles the row's end -- on the frame's last row, the span's end -- and the range check would drop it whole, so the read
// descriptor gets 3 extra records (fused_geom's rule) when reading them is safe: behind every frame but the last they lie in
// the next frame or the stride padding, behind the last frame they must stay in the 4-KiB page of its last byte.
inline PitchedPlan pitched_plan(uint64_t src, const PitchedFrames &f, bool force_checked)
{
    PitchedPlan p = {};
    p.W = f.width;
    p.H = f.height;
    p.tx = (uint32_t)(((uint64_t)f.width + kPitchedTileW - 1) / kPitchedTileW);
    p.ty = (uint32_t)(((uint64_t)f.height + kPitchedTileH - 1) / kPitchedTileH);
    p.sp = f.height > 1 ? f.src_pitch : f.width;
    p.dp = f.height > 1 ? f.dst_pitch : f.width;
    p.sstride = f.batch > 1 ? f.src_stride : 0;
    p.dstride = f.batch > 1 ? f.dst_stride : 0;
    const uint64_t sspan = pitched_span(f.width, f.height, p.sp), dspan = pitched_span(f.width, f.height, p.dp);
    // every 32-bit buffer offset the fast path forms: (Y0 + TH + 64) * pitch + X0 + TW + 64 + 16, Y0 + TH <= H + TH
    const uint64_t maxp = p.sp > p.dp ? p.sp : p.dp;
    const bool fits32 = maxp < (1ull << 32) && ((uint64_t)f.height + 2 * kPitchedTileH + 64) * maxp + 1024 < (1ull << 32);
    const bool dword_rows = f.width % 4 == 0;
    const uint64_t end = src + (uint64_t)(f.batch - 1) * p.sstride + sspan;
    const bool tail_ok = ((end - 1) >> 12) == ((end + 2) >> 12) && (f.batch == 1 || p.sstride >= sspan);
    p.fast = fits32 && (dword_rows || tail_ok) && !force_checked ? 1u : 0u;
    p.sp32 = p.fast ? (uint32_t)p.sp : 0u;
    p.dp32 = p.fast ? (uint32_t)p.dp : 0u;
    p.srec = p.fast ? (uint32_t)sspan + (dword_rows ? 0u : 3u) : 0u;
    p.drec = p.fast ? (uint32_t)dspan : 0u;
    p.ix = p.fast ? f.width / kPitchedTileW : 0u;
    p.iy = p.fast ? f.height / kPitchedTileH : 0u;
    if (p.ix == 0 || p.iy == 0) p.ix = p.iy = 0;
    p.ipf = p.ix * p.iy;
    const uint64_t tpf = (uint64_t)p.tx * p.ty, nf = (uint64_t)p.ipf * f.batch, ne = (tpf - p.ipf) * f.batch;
    p.ok = tpf > 0 && f.batch > 0 && tpf < (1ull << 31) && nf + ne + 8 < (1ull << 31);
    p.epf = p.ok ? (uint32_t)(tpf - p.ipf) : 0u;
    p.nf = p.ok ? (uint32_t)nf : 0u;
    p.nedge = p.ok ? (uint32_t)ne : 0u;
    p.fd_ix = make_fastdiv(p.ix ? p.ix : 1u);
    p.fd_ipf = make_fastdiv(p.ipf ? p.ipf : 1u);
    return p;
}

HGI_HD inline uint64_t pitched_blocks(const PitchedPlan &p) { return (((uint64_t)p.nedge + 7u) & ~(uint64_t)7u) + p.nf; }

struct PitchedTile {
    uint32_t frame, X0, Y0;
    bool edge, idle;
};

// x-th contiguous eighth of n tiles (range_first of hgi_fused_impl.h)
HGI_HD inline uint32_t pitched_eighth(uint32_t n, uint32_t x) { return x * (n >> 3) + (x < (n & 7u) ? x : (n & 7u)); }

// Block b of the launch -> its tile.
HGI_HD inline PitchedTile pitched_tile(const PitchedPlan &p, uint32_t b)
{
    const uint32_t ne8 = (p.nedge + 7u) & ~7u;
    PitchedTile t;
    uint32_t tx, ty;
    t.edge = b < ne8;
    t.idle = t.edge && b >= p.nedge;
    if (t.edge) {
        const uint32_t e = t.idle ? 0u : b;
        t.frame = e / p.epf;
        uint32_t i = e - t.frame * p.epf;
        const uint32_t right = (p.tx - p.ix) * p.ty;      // tiles with tx >= ix
        if (i < right) {
            const uint32_t w = p.tx - p.ix;
            ty = i / w;
            tx = p.ix + (i - ty * w);
        } else {                                          // tiles with ty >= iy, tx < ix
            i -= right;
            ty = p.iy + i / p.ix;
            tx = i % p.ix;
        }
    } else {
        const uint32_t fb = b - ne8;
        const uint32_t i = pitched_eighth(p.nf, fb & 7u) + (fb >> 3);
        t.frame = fdiv(i, p.fd_ipf);
        const uint32_t r = i - t.frame * p.ipf;
        ty = fdiv(r, p.fd_ix);
        tx = r - ty * p.ix;
    }
    t.X0 = tx * kPitchedTileW;
    t.Y0 = ty * kPitchedTileH;
    return t;
}

}  // namespace hgi
