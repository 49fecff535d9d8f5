// What the companion libraries (../recon, ../map, ../typed, ../requant) share on the host, on top of the pitched plan
// (csrc/hgi_pitched.h): the 32-bit bound of a side, the page rule of the bytes read behind the last frame, the byte intervals
// of a call's aliasing test, the split of the pyramid and the kernel argument of a launch's extra side.  One copy: a change of
// the tile procedure's largest offset is made here.  Plain C++: tests/cpp/test_sides.cpp runs it with g++.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../csrc/hgi_pitched.h"

namespace hgi {

// Every 32-bit buffer offset the tile procedure forms on a side whose rows lie `pitch` bytes apart stays below 2^32
// (pitched_plan's bound).  The largest offset each user forms, Y0 <= height and X0 + 128 <= 2^32 / pitch:
//   * pitched u8 sides (recon's three, requant's two, the grids of map and typed): (Y0 + 64 + 64) * pitch + X0 + 128 + 64 + 16;
//   * the mapped output, E-byte elements: (Y0 + 64) * pitch + (X0 + 128) * E <= (height + 65) * pitch + 512;
//   * the typed image, E-byte elements: (Y0 + 64 + 64) * pitch + (X0 + 128 + 64 + 16) * E <= (height + 129) * pitch + 832.
inline bool side_fits32(uint32_t height, uint64_t pitch)
{
    return pitch < (1ull << 32) && ((uint64_t)height + 2 * kPitchedTileH + 64) * pitch + 1024 < (1ull << 32);
}

// Bytes from a frame's first byte to its last, rows of `row_bytes` bytes.
inline uint64_t side_span(uint64_t row_bytes, uint32_t height, uint64_t pitch) { return (uint64_t)(height - 1) * pitch + row_bytes; }

// The `extra` bytes read behind the last frame's span lie in the 4-KiB page of the span's last byte, and the frames in front
// of it are at least a span apart (the bytes behind them lie in the next frame or the stride padding).  `pitch` and `stride`
// as given by the caller: a one-row frame never steps by its pitch, a single frame never by its stride.
inline bool tail_in_page(uint64_t first_frame, uint64_t row_bytes, uint32_t h, uint64_t pitch, uint64_t stride, uint32_t batch, uint32_t extra)
{
    const uint64_t st = batch > 1 ? stride : 0;
    const uint64_t span = side_span(row_bytes, h, h > 1 ? pitch : row_bytes);
    const uint64_t end = first_frame + (uint64_t)(batch - 1) * st + span;
    return ((end - 1) >> 12) == ((end - 1 + extra) >> 12) && (batch == 1 || st >= span);
}

// ---- byte intervals of a call: first byte of the first frame to last byte of the last --------------------------------------
struct Interval {
    unsigned __int128 lo, hi;     // [lo, hi)
};

inline Interval side_interval(uint64_t ptr, uint64_t row_bytes, uint32_t h, uint64_t pitch, uint64_t stride, uint64_t batch)
{
    typedef unsigned __int128 u128;
    const u128 span = (u128)(h - 1) * pitch + row_bytes;
    Interval i;
    i.lo = ptr;
    i.hi = (u128)ptr + (u128)(batch - 1) * (batch > 1 ? stride : 0) + span;
    return i;
}

inline Interval table_interval(uint64_t ptr, uint64_t bytes)
{
    Interval i;
    i.lo = ptr;
    i.hi = (unsigned __int128)ptr + bytes;
    return i;
}

inline bool meet(const Interval &a, const Interval &b) { return a.lo < b.hi && b.lo < a.hi; }

// How the pyramid is split between the tile and the cone: libhgi_hip.so's rule for one launch (csrc/hgi_capi.hip,
// split_pyramid): up to five levels the tile holds the pyramid, six to eight are four fused levels under a cone.
inline void split_levels(uint32_t levels, uint32_t *k, uint32_t *up)
{
    *k = levels < 6u ? levels : 4u;
    *up = levels < 6u ? 0u : levels - 4u;
}

// The side a launch has beside the two of its PitchedPlan (kernel argument, by value): the 32-bit pitch and the num_records
// of its descriptor -- both 0 on a plan that is not `fast` -- and the bytes between its frames.
struct ExtraSide {
    uint32_t pitch32, rec;
    uint64_t stride;
};

// A plan with an extra side is {PitchedPlan p; ExtraSide x;}: the layout the kernels were compiled against when the three
// members stood in the plan itself -- {PitchedPlan p; uint32_t pitch32, rec; uint64_t stride;} -- member by member.
template <class Plan>
constexpr bool extra_side_layout()
{
    return sizeof(Plan) == sizeof(PitchedPlan) + 16 && alignof(Plan) == 8 && sizeof(PitchedPlan) % 8 == 0 && offsetof(Plan, p) == 0 &&
           offsetof(Plan, x.pitch32) == sizeof(PitchedPlan) && offsetof(Plan, x.rec) == sizeof(PitchedPlan) + 4 &&
           offsetof(Plan, x.stride) == sizeof(PitchedPlan) + 8;
}

inline ExtraSide extra_side(bool fast, uint64_t pitch, uint64_t span_plus_tail, uint64_t stride)
{
    const ExtraSide x = {fast ? (uint32_t)pitch : 0u, fast ? (uint32_t)span_plus_tail : 0u, stride};
    return x;
}

}  // namespace hgi
