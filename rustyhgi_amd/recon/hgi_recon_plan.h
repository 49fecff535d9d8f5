// Encode with reconstruction (hgi_recon_encode_u8_dev, include/hgi_recon.h): the host plan of the three-sided launch -- the
// image read, the grid and the reconstruction written, each side with a pitch and a frame stride of its own.  The bound of a
// side, the page rule and the byte-interval tests of the call are companion/hgi_sides.h's.  On top of the pitched plan
// (csrc/hgi_pitched.h): the tile list, the block -> tile map and the launch order are pitched_plan's / pitched_tile's as they
// stand; this adds the third side.  Plain C++: tests/cpp/test_recon_plan.cpp runs it with g++.
//
// This library has no byte-checked path: a call whose three sides do not all take the 32-bit buffer path is refused
// (HGI_EUNSUPPORTED) and the caller composes hgi_encode_u8_dev + hgi_decode_u8_dev instead.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../companion/hgi_sides.h"

namespace hgi {

struct ReconFrames {
    uint32_t width, height, batch;
    uint64_t img_pitch, grid_pitch, recon_pitch;        // bytes between rows
    uint64_t img_stride, grid_stride, recon_stride;     // bytes between frames
};

// What a launch reads (kernel argument, by value): the pitched plan of (image -> grid) and the reconstruction's side.
struct ReconPlan {
    PitchedPlan p;
    ExtraSide x;                  // the reconstruction: write pitch, num_records (span) of its descriptor, frame stride
};
static_assert(extra_side_layout<ReconPlan>(), "a kernel argument: its layout is the kernels'");

// What the host decides on: the plan, and why its `p.fast` is what it is.
struct ReconJudged {
    ReconPlan plan;
    uint64_t rp;                  // the reconstruction's pitch (a one-row frame's counts as its width)
    bool fits32, tail_ok;
};

// img: address of the first input frame.  width, height, batch >= 1.
inline ReconJudged recon_plan(uint64_t img, const ReconFrames &f)
{
    ReconJudged r = {};
    const PitchedFrames pf = {f.width, f.height, f.batch, f.img_pitch, f.grid_pitch, f.img_stride, f.grid_stride};
    r.rp = f.height > 1 ? f.recon_pitch : f.width;
    // `fast` holds only if all three sides fit: the pitched plan judges two of them, and is made as the checked plan (no 32-bit
    // pitches, no records, no interior tiles) when the third fails, so that it never describes a buffer path that does not exist
    r.plan.p = pitched_plan(img, pf, !side_fits32(f.height, r.rp));
    r.fits32 = side_fits32(f.height, r.plan.p.sp) && side_fits32(f.height, r.plan.p.dp) && side_fits32(f.height, r.rp);
    // the three tail bytes behind the last input frame's span are asked for only when width % 4 != 0: the dword that holds a
    // row's last bytes straddles the span's end on the last row of the last frame
    r.tail_ok = f.width % 4 == 0 || tail_in_page(img, f.width, f.height, f.img_pitch, f.img_stride, f.batch, 3);
    r.plan.x = extra_side(r.plan.p.fast, r.rp, side_span(f.width, f.height, r.rp), f.batch > 1 ? f.recon_stride : 0);
    return r;
}

}  // namespace hgi
