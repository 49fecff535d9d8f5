// Requantize (hgi_requant_dev, include/hgi_requant.h): the host plan of the two-sided launch -- the source grid read, the new
// grid written, each side with a pitch and a frame stride of its own.  The bound of a side, the page rule and the byte-interval
// test of the call are companion/hgi_sides.h's.  On top of the pitched plan (csrc/hgi_pitched.h): the tile list, the block -> tile map, the 32-bit pitches, the descriptors' records and the
// strides of both sides are pitched_plan's as they stand; this adds why its `fast` is what it is (which side does not fit, the
// tail rule on the source side), so that the entry point can say so.  Plain C++: tests/cpp/test_requant_plan.cpp runs it with g++.
//
// This library has no byte-checked path: a call whose two sides do not both take the 32-bit buffer path is refused
// (HGI_EUNSUPPORTED) and the caller composes hgi_decode_u8_dev + hgi_encode_u8_dev instead.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../companion/hgi_sides.h"

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

// src: address of the first source frame.  width, height, batch >= 1.  plan.fast holds only if both sides fit and the tail rule
// holds; otherwise the plan is the checked one (no 32-bit pitches, no records, no interior tiles) and is never launched.
inline RequantJudged requant_plan(uint64_t src, const RequantFrames &f)
{
    RequantJudged r = {};
    const PitchedFrames pf = {f.width, f.height, f.batch, f.src_pitch, f.dst_pitch, f.src_stride, f.dst_stride};
    r.plan = pitched_plan(src, pf, false);
    r.fits32 = side_fits32(f.height, r.plan.sp) && side_fits32(f.height, r.plan.dp);
    // the three tail bytes behind the last SOURCE frame's span are asked for only when width % 4 != 0: the dword that holds a
    // row's last bytes straddles the span's end on the last row of the last frame
    r.tail_ok = f.width % 4 == 0 || tail_in_page(src, f.width, f.height, f.src_pitch, f.src_stride, f.batch, 3);
    return r;
}

}  // namespace hgi
