// Requantize (hgi_requant_dev, include/hgi_requant.h): the host plan of the two-sided launch -- the source grid read, the new
// grid written, each side with a pitch and a frame stride of its own -- and the byte interval test of the call.  On top of the
// pitched plan (csrc/hgi_pitched.h): the tile list, the block -> tile map, the 32-bit pitches, the descriptors' records and the
// strides of both sides are pitched_plan's as they stand; this adds why its `fast` is what it is (which side does not fit, the
// tail rule on the source side), so that the entry point can say so.  Plain C++: tests/cpp/test_requant_plan.cpp runs it with g++.
//
// This library has no byte-checked path: a call whose two sides do not both take the 32-bit buffer path is refused
// (HGI_EUNSUPPORTED) and the caller composes hgi_decode_u8_dev + hgi_encode_u8_dev instead.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../csrc/hgi_pitched.h"

namespace hgi {

struct RequantFrames {
    uint32_t width, height, batch;
    uint64_t src_pitch, dst_pitch;        // bytes between rows
    uint64_t src_stride, dst_stride;      // bytes between frames
};

// What the host decides on: the plan a launch reads (kernel argument, by value), and why its `fast` is what it is.
struct RequantJudged {
    PitchedPlan plan;
    bool fits32, tail_ok;
};

// Every 32-bit buffer offset the tile procedure forms on a side whose rows lie `pitch` bytes apart (pitched_plan's bound).
inline bool requant_fits32(uint32_t height, uint64_t pitch)
{
    return pitch < (1ull << 32) && ((uint64_t)height + 2 * kPitchedTileH + 64) * pitch + 1024 < (1ull << 32);
}

// The three tail bytes behind the last SOURCE frame's span lie in the 4-KiB page of the span's last byte (asked for only when
// width % 4 != 0: the dword that holds a row's last bytes straddles the span's end on the last row of the last frame).
inline bool requant_tail_ok(uint64_t src, const RequantFrames &f)
{
    const uint64_t sp = f.height > 1 ? f.src_pitch : f.width, stride = f.batch > 1 ? f.src_stride : 0;
    const uint64_t span = pitched_span(f.width, f.height, sp);
    const uint64_t end = src + (uint64_t)(f.batch - 1) * stride + span;
    return ((end - 1) >> 12) == ((end + 2) >> 12) && (f.batch == 1 || stride >= span);
}

// src: address of the first source frame.  width, height, batch >= 1.  plan.fast holds only if both sides fit and the tail rule
// holds; otherwise the plan is the checked one (no 32-bit pitches, no records, no interior tiles) and is never launched.
inline RequantJudged requant_plan(uint64_t src, const RequantFrames &f)
{
    RequantJudged r = {};
    const PitchedFrames pf = {f.width, f.height, f.batch, f.src_pitch, f.dst_pitch, f.src_stride, f.dst_stride};
    r.plan = pitched_plan(src, pf, false);
    r.fits32 = requant_fits32(f.height, r.plan.sp) && requant_fits32(f.height, r.plan.dp);
    r.tail_ok = f.width % 4 == 0 || requant_tail_ok(src, f);
    return r;
}

// ---- byte intervals of a call (computed as in the pitched calls: first byte of the first frame to last byte of the last) ----
struct RequantInterval {
    unsigned __int128 lo, hi;     // [lo, hi)
};

inline RequantInterval requant_interval(uint64_t ptr, uint32_t w, uint32_t h, uint64_t pitch, uint64_t stride, uint64_t batch)
{
    typedef unsigned __int128 u128;
    const u128 span = (u128)(h - 1) * pitch + w;
    RequantInterval i;
    i.lo = ptr;
    i.hi = (u128)ptr + (u128)(batch - 1) * (batch > 1 ? stride : 0) + span;
    return i;
}

inline bool requant_meet(const RequantInterval &a, const RequantInterval &b) { return a.lo < b.hi && b.lo < a.hi; }

}  // namespace hgi
