// Encode with reconstruction (hgi_recon_encode_u8_dev, include/hgi_recon.h): the host plan of the three-sided launch -- the
// image read, the grid and the reconstruction written, each side with a pitch and a frame stride of its own -- and the byte
// interval tests of the call.  On top of the pitched plan (csrc/hgi_pitched.h): the tile list, the block -> tile map and the
// launch order are pitched_plan's / pitched_tile's as they stand; this adds the third side.  Plain C++:
// tests/cpp/test_recon_plan.cpp runs it with g++.
//
// This library has no byte-checked path: a call whose three sides do not all take the 32-bit buffer path is refused
// (HGI_EUNSUPPORTED) and the caller composes hgi_encode_u8_dev + hgi_decode_u8_dev instead.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../csrc/hgi_pitched.h"

namespace hgi {

struct ReconFrames {
    uint32_t width, height, batch;
    uint64_t img_pitch, grid_pitch, recon_pitch;        // bytes between rows
    uint64_t img_stride, grid_stride, recon_stride;     // bytes between frames
};

// What a launch reads (kernel argument, by value): the pitched plan of (image -> grid) and the reconstruction's side.
struct ReconPlan {
    PitchedPlan p;
    uint32_t rp32, rrec;          // write pitch and num_records (span) of the reconstruction's descriptor
    uint64_t rstride;
};

// What the host decides on: the plan, and why its `p.fast` is what it is.
struct ReconJudged {
    ReconPlan plan;
    uint64_t rp;                  // the reconstruction's pitch (a one-row frame's counts as its width)
    bool fits32, tail_ok;
};

// Every 32-bit buffer offset the tile procedure forms on a side whose rows lie `pitch` bytes apart (pitched_plan's bound).
inline bool recon_fits32(uint32_t height, uint64_t pitch)
{
    return pitch < (1ull << 32) && ((uint64_t)height + 2 * kPitchedTileH + 64) * pitch + 1024 < (1ull << 32);
}

// The three tail bytes behind the last input frame's span lie in the 4-KiB page of the span's last byte (asked for only
// when width % 4 != 0: the dword that holds a row's last bytes straddles the span's end on the last row of the last frame).
inline bool recon_tail_ok(uint64_t img, const ReconFrames &f)
{
    const uint64_t sp = f.height > 1 ? f.img_pitch : f.width, stride = f.batch > 1 ? f.img_stride : 0;
    const uint64_t span = pitched_span(f.width, f.height, sp);
    const uint64_t end = img + (uint64_t)(f.batch - 1) * stride + span;
    return ((end - 1) >> 12) == ((end + 2) >> 12) && (f.batch == 1 || stride >= span);
}

// img: address of the first input frame.  width, height, batch >= 1.
inline ReconJudged recon_plan(uint64_t img, const ReconFrames &f)
{
    ReconJudged r = {};
    const PitchedFrames pf = {f.width, f.height, f.batch, f.img_pitch, f.grid_pitch, f.img_stride, f.grid_stride};
    r.rp = f.height > 1 ? f.recon_pitch : f.width;
    // `fast` holds only if all three sides fit: the pitched plan judges two of them, and is made as the checked plan (no 32-bit
    // pitches, no records, no interior tiles) when the third fails, so that it never describes a buffer path that does not exist
    r.plan.p = pitched_plan(img, pf, !recon_fits32(f.height, r.rp));
    r.plan.rstride = f.batch > 1 ? f.recon_stride : 0;
    r.fits32 = recon_fits32(f.height, r.plan.p.sp) && recon_fits32(f.height, r.plan.p.dp) && recon_fits32(f.height, r.rp);
    r.tail_ok = f.width % 4 == 0 || recon_tail_ok(img, f);
    r.plan.rp32 = r.plan.p.fast ? (uint32_t)r.rp : 0u;
    r.plan.rrec = r.plan.p.fast ? (uint32_t)pitched_span(f.width, f.height, r.rp) : 0u;
    return r;
}

// ---- byte intervals of a call (computed as in the pitched calls: first byte of the first frame to last byte of the last) ----
struct ReconInterval {
    unsigned __int128 lo, hi;     // [lo, hi)
};

inline ReconInterval recon_interval(uint64_t ptr, uint32_t w, uint32_t h, uint64_t pitch, uint64_t stride, uint64_t batch)
{
    typedef unsigned __int128 u128;
    const u128 span = (u128)(h - 1) * pitch + w;
    ReconInterval i;
    i.lo = ptr;
    i.hi = (u128)ptr + (u128)(batch - 1) * (batch > 1 ? stride : 0) + span;
    return i;
}

inline bool recon_meet(const ReconInterval &a, const ReconInterval &b) { return a.lo < b.hi && b.lo < a.hi; }

}  // namespace hgi
