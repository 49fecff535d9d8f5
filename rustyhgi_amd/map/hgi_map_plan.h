// Mapped decode (hgi_map_decode_dev, include/hgi_map.h): the host plan of the launch -- the grid read through its pitch, the
// output of E-byte elements written through a BYTE pitch of its own.  The bound of a side, the page rule and the byte-interval
// tests of the call are companion/hgi_sides.h's.  On top of the pitched plan (csrc/hgi_pitched.h): pitched_plan judges the grid
// side and owns the tile list, the block -> tile map and the launch order as they stand; this adds the output side.  Plain
// C++: tests/cpp/test_map_plan.cpp runs it with g++.
//
// This library has no byte-checked path: a call whose two sides do not both take the 32-bit buffer path is refused
// (HGI_EUNSUPPORTED) and the caller composes hgi_decode_u8_pitched_dev + a gather instead.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../companion/hgi_sides.h"

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
    ExtraSide x;                  // the output: write pitch, num_records (span) of its descriptor, frame stride, bytes
};
static_assert(extra_side_layout<MapPlan>(), "a kernel argument: its layout is the kernels'");

// What the host decides on: the plan, and why its `p.fast` is what it is.
struct MapJudged {
    MapPlan plan;
    uint64_t op, ospan;           // the output's pitch (a one-row frame's counts as its row) and span, bytes
    bool fits32, tail_ok;
};

// grid: address of the first grid frame.  width, height, batch >= 1; elem 2 or 4.
inline MapJudged map_plan(uint64_t grid, const MapFrames &f)
{
    MapJudged r = {};
    const PitchedFrames pf = {f.width, f.height, f.batch, f.grid_pitch, f.grid_pitch, f.grid_stride, f.grid_stride};
    r.op = f.height > 1 ? f.out_pitch : (uint64_t)f.width * f.elem;
    r.ospan = side_span((uint64_t)f.width * f.elem, f.height, r.op);
    // `fast` holds only if both sides fit: the pitched plan judges the grid side, and is made as the checked plan (no 32-bit
    // pitches, no records, no interior tiles) when the output side fails, so that it never describes a buffer path that does
    // not exist
    r.plan.p = pitched_plan(grid, pf, !side_fits32(f.height, r.op));
    r.fits32 = side_fits32(f.height, r.plan.p.sp) && side_fits32(f.height, r.op);
    // the three tail bytes behind the last grid frame's span are asked for only when width % 4 != 0: the dword that holds a
    // row's last bytes straddles the span's end on the last row of the last frame
    r.tail_ok = f.width % 4 == 0 || tail_in_page(grid, f.width, f.height, f.grid_pitch, f.grid_stride, f.batch, 3);
    r.plan.x = extra_side(r.plan.p.fast, r.op, r.ospan, f.batch > 1 ? f.out_stride : 0);
    return r;
}

}  // namespace hgi
