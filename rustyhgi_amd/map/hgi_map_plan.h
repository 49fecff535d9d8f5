// Mapped decode (hgi_map_decode_dev, include/hgi_map.h): the host plan of the launch -- the grid read through its pitch, the
// output of E-byte elements written through a BYTE pitch of its own -- and the byte-interval tests of the call.  On top of
// the pitched plan (csrc/hgi_pitched.h): pitched_plan judges the grid side and owns the tile list, the block -> tile map and
// the launch order as they stand; this adds the output side.  Plain C++: tests/cpp/test_map_plan.cpp runs it with g++.
//
// This library has no byte-checked path: a call whose two sides do not both take the 32-bit buffer path is refused
// (HGI_EUNSUPPORTED) and the caller composes hgi_decode_u8_pitched_dev + a gather instead.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../csrc/hgi_pitched.h"

namespace hgi {

struct MapFrames {
    uint32_t width, height, batch, elem;      // elem: bytes per output element (2 or 4)
    uint64_t grid_pitch, out_pitch;           // bytes between rows
    uint64_t grid_stride, out_stride;         // bytes between frames
};

// What a launch reads (kernel argument, by value): the pitched plan of the grid side (its write side mirrors the read side and
// is not used) and the output's side.
struct MapPlan {
    PitchedPlan p;
    uint32_t op32, orec;          // write pitch and num_records (span) of the output's descriptor, bytes
    uint64_t ostride;
};

// What the host decides on: the plan, and why its `p.fast` is what it is.
struct MapJudged {
    MapPlan plan;
    uint64_t op, ospan;           // the output's pitch (a one-row frame's counts as its row) and span, bytes
    bool fits32, tail_ok;
};

// Every 32-bit buffer offset the tile procedure forms on a side whose rows lie `pitch` bytes apart (pitched_plan's bound; on
// the output side the largest is (Y0 + 64) * pitch + (X0 + 128) * E <= (height + 65) * pitch + 512).
inline bool map_fits32(uint32_t height, uint64_t pitch)
{
    return pitch < (1ull << 32) && ((uint64_t)height + 2 * kPitchedTileH + 64) * pitch + 1024 < (1ull << 32);
}

// Bytes from an output frame's first byte to its last.
inline uint64_t map_out_span(uint32_t w, uint32_t h, uint32_t elem, uint64_t pitch) { return (uint64_t)(h - 1) * pitch + (uint64_t)w * elem; }

// The three tail bytes behind the last grid frame's span lie in the 4-KiB page of the span's last byte (asked for only when
// width % 4 != 0: the dword that holds a row's last bytes straddles the span's end on the last row of the last frame).
inline bool map_tail_ok(uint64_t grid, const MapFrames &f)
{
    const uint64_t sp = f.height > 1 ? f.grid_pitch : f.width, stride = f.batch > 1 ? f.grid_stride : 0;
    const uint64_t span = pitched_span(f.width, f.height, sp);
    const uint64_t end = grid + (uint64_t)(f.batch - 1) * stride + span;
    return ((end - 1) >> 12) == ((end + 2) >> 12) && (f.batch == 1 || stride >= span);
}

// grid: address of the first grid frame.  width, height, batch >= 1; elem 2 or 4.
inline MapJudged map_plan(uint64_t grid, const MapFrames &f)
{
    MapJudged r = {};
    const PitchedFrames pf = {f.width, f.height, f.batch, f.grid_pitch, f.grid_pitch, f.grid_stride, f.grid_stride};
    r.op = f.height > 1 ? f.out_pitch : (uint64_t)f.width * f.elem;
    r.ospan = map_out_span(f.width, f.height, f.elem, r.op);
    // `fast` holds only if both sides fit: the pitched plan judges the grid side, and is made as the checked plan (no 32-bit
    // pitches, no records, no interior tiles) when the output side fails, so that it never describes a buffer path that does
    // not exist
    r.plan.p = pitched_plan(grid, pf, !map_fits32(f.height, r.op));
    r.plan.ostride = f.batch > 1 ? f.out_stride : 0;
    r.fits32 = map_fits32(f.height, r.plan.p.sp) && map_fits32(f.height, r.op);
    r.tail_ok = f.width % 4 == 0 || map_tail_ok(grid, f);
    r.plan.op32 = r.plan.p.fast ? (uint32_t)r.op : 0u;
    r.plan.orec = r.plan.p.fast ? (uint32_t)r.ospan : 0u;
    return r;
}

// ---- byte intervals of a call: first byte of the first frame to last byte of the last; `row` bytes per row ----------------
struct MapInterval {
    unsigned __int128 lo, hi;     // [lo, hi)
};

inline MapInterval map_interval(uint64_t ptr, uint64_t row, uint32_t h, uint64_t pitch, uint64_t stride, uint64_t batch)
{
    typedef unsigned __int128 u128;
    const u128 span = (u128)(h - 1) * pitch + row;
    MapInterval i;
    i.lo = ptr;
    i.hi = (u128)ptr + (u128)(batch - 1) * (batch > 1 ? stride : 0) + span;
    return i;
}

// the table: 256 elements of `elem` bytes
inline MapInterval map_table_interval(uint64_t ptr, uint32_t elem)
{
    MapInterval i;
    i.lo = ptr;
    i.hi = (unsigned __int128)ptr + 256u * (uint64_t)elem;
    return i;
}

inline bool map_meet(const MapInterval &a, const MapInterval &b) { return a.lo < b.hi && b.lo < a.hi; }

}  // namespace hgi
