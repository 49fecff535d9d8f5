// Typed encode (hgi_typed_encode_dev, include/hgi_typed.h): the host plan of the launch -- the image of E-byte elements read
// through a BYTE pitch of its own, the grid written through its pitch.  The bound of a side, the page rule and the byte-interval
// test of the call are companion/hgi_sides.h's.  On top of the pitched plan (csrc/hgi_pitched.h): pitched_plan judges the grid side in pixels and owns the tile list, the block -> tile map
// and the launch order as they stand; this adds the image side in bytes.  Plain C++: tests/cpp/test_typed_plan.cpp runs it
// with g++.
//
// This library has no byte-checked path: a call whose two sides do not both take the 32-bit buffer path is refused
// (HGI_EUNSUPPORTED) and the caller composes a conversion + hgi_encode_u8_pitched_dev instead.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../companion/hgi_sides.h"

namespace hgi {

struct TypedFrames {
    uint32_t width, height, batch, elem;      // elem: bytes per image element (2 or 4)
    uint64_t img_pitch, grid_pitch;           // bytes between rows
    uint64_t img_stride, grid_stride;         // bytes between frames
};

// What a launch reads (kernel argument, by value): the pitched plan of the grid side (its read side mirrors the write side and
// is not used) and the image's side.
struct TypedPlan {
    PitchedPlan p;
    ExtraSide x;                  // the image: read pitch, num_records (span + tail) of its descriptor, frame stride, bytes
};
static_assert(extra_side_layout<TypedPlan>(), "a kernel argument: its layout is the kernels'");

// What the host decides on: the plan, and why its `p.fast` is what it is.
struct TypedJudged {
    TypedPlan plan;
    uint64_t ip, ispan;           // the image's pitch (a one-row frame's counts as its row) and span, bytes
    bool fits32, tail_ok;
};

// E = 2 and an odd width: the dword that holds a row's last element straddles the row's end -- on the last row, the span's end
// -- and the range check would drop it whole, so the descriptor gets 2 extra records.  Behind every frame but the last they lie
// in the next frame or the stride padding; behind the last frame they must stay in the 4-KiB page of its last byte, i.e. the
// span must not end on a page boundary.  E = 4: dwords of 4-byte-aligned elements never straddle the span's end.
inline bool typed_tail_needed(const TypedFrames &f) { return f.elem == 2 && (f.width & 1u); }

// The pitched plan of a side that is only WRITTEN.  pitched_plan takes the address of the side it READS, for one purpose: its
// rule about the three bytes read behind the last frame's span (widths that are no multiple of 4).  The grid of a typed encode
// is never read, so that rule has no subject here, and csrc/hgi_pitched.h -- part of libhgi_hip.so's hashed sources -- offers
// no switch for it.  This is the one place that knows how to ask for a plan without it: at an address where the last frame's
// span ends 8 bytes into a page the rule holds for every shape.  tests/cpp/test_typed_plan.cpp holds `fast` to the typed rules
// alone at every width class and image address.
inline PitchedPlan typed_grid_plan(const PitchedFrames &pf, bool force_checked)
{
    const uint64_t gp = pf.height > 1 ? pf.dst_pitch : pf.width, gstride = pf.batch > 1 ? pf.dst_stride : 0;
    const uint64_t total = (uint64_t)(pf.batch - 1) * gstride + pitched_span(pf.width, pf.height, gp);
    return pitched_plan(8 - total, pf, force_checked);      // (mod 2^64: only the address's place in its page is looked at)
}

// img: address of the first image frame.  width, height, batch >= 1; elem 2 or 4.
inline TypedJudged typed_plan(uint64_t img, const TypedFrames &f)
{
    TypedJudged r = {};
    const PitchedFrames pf = {f.width, f.height, f.batch, f.grid_pitch, f.grid_pitch, f.grid_stride, f.grid_stride};
    r.ip = f.height > 1 ? f.img_pitch : (uint64_t)f.width * f.elem;
    r.ispan = side_span((uint64_t)f.width * f.elem, f.height, r.ip);
    const uint64_t gp = f.height > 1 ? f.grid_pitch : f.width;
    r.fits32 = side_fits32(f.height, gp) && side_fits32(f.height, r.ip);
    r.tail_ok = !typed_tail_needed(f) || tail_in_page(img, (uint64_t)f.width * f.elem, f.height, f.img_pitch, f.img_stride, f.batch, 2);
    // `fast` holds only if both sides fit and the image's tail rule holds: the pitched plan is made as the checked plan (no
    // 32-bit pitches, no records, no interior tiles) otherwise, so that it never describes a buffer path that does not exist.
    r.plan.p = typed_grid_plan(pf, !(r.fits32 && r.tail_ok));
    r.plan.x = extra_side(r.plan.p.fast, r.ip, r.ispan + (typed_tail_needed(f) ? 2u : 0u), f.batch > 1 ? f.img_stride : 0);
    return r;
}

}  // namespace hgi
