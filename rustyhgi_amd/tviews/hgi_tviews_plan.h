// Typed view lists (hgi_tviews_plan / hgi_tviews_encode_dev, include/hgi_tviews.h): the host plan of one launch over the
// 128 x 64 tiles of many frames of E-byte elements that each bring a shape, a BYTE pitch and -- for the grid that is written --
// a pitch of their own.  It is the view lists' plan (../views/hgi_views_plan.h) with the read side in bytes:
//   * the record is that plan's 64-byte ViewFrame; per entry it is typed_plan (../typed/hgi_typed_plan.h) of a batch of one,
//     field by field: the written side and the tile counts from its pitched plan of the grid (asked for the way typed_grid_plan
//     asks, the grid is never read), on the read side sp32 the frame's byte pitch and srec the span (h - 1) * pitch + w * E,
//     plus 2 where E = 2 and the width is odd -- its ExtraSide;
//   * the blob, the launch order, the block -> tile map and the frame search are the view lists' unchanged (view_block,
//     views_blob_bytes, the offsets);
//   * the rules of a list are the view lists' plus those of E-byte elements; the aliasing test is the mapped view lists' sweep
//     on rectangles of bytes with 64-bit rows (../mviews/hgi_mviews_plan.h: MViewRect, mview_rect, mviews_aliasing), used by
//     inclusion with the sides swapped: here the grids are the outputs and the frames, w * E bytes wide, the inputs.
// Plain C++: tests/cpp/test_tviews_plan.cpp runs it with g++.
//
// This library has no byte-checked path: a list with an entry that does not take the 32-bit buffer path is refused
// (HGI_EUNSUPPORTED) and the caller composes one typed encode per view.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/hgi_tviews.h"
#include "../mviews/hgi_mviews_plan.h"
#include "../typed/hgi_typed_plan.h"

namespace hgi {

// ---- per-frame geometry: typed_plan of a batch of one --------------------------------------------------------------------------
inline TypedJudged tview_typed_plan(const hgi_tview_pair &v, uint32_t elem)
{
    const TypedFrames f = {v.width, v.height, 1u, elem, v.src_pitch, v.dst_pitch, 0, 0};
    return typed_plan(v.src, f);
}

// `t`: tview_typed_plan(v) of an entry that passed every rule (t.plan.p.fast holds).
inline ViewFrame tview_frame(const hgi_tview_pair &v, const TypedPlan &t)
{
    const hgi_view_pair u = {v.src, v.dst, v.width, v.height, v.src_pitch, v.dst_pitch};
    ViewFrame f = view_frame(u, t.p);
    f.sp32 = t.x.pitch32;
    f.srec = t.x.rec;
    return f;
}

// The three arrays of a blob that lies at `base`, per `info` (view_args on this library's struct).
inline ViewArgs tview_args(const void *base, const hgi_tviews_info &info)
{
    const uint8_t *b = static_cast<const uint8_t *>(base);
    ViewArgs a;
    a.frames = reinterpret_cast<const ViewFrame *>(b + info.records_offset);
    a.epre = reinterpret_cast<const uint32_t *>(b + info.edge_prefix_offset);
    a.ipre = reinterpret_cast<const uint32_t *>(b + info.interior_prefix_offset);
    a.count = info.count;
    a.nedge = info.edge_tiles;
    a.nint = info.interior_tiles;
    return a;
}

// What a launch checks of the host struct it is handed: the magic, the element size, the sizes and offsets against the count,
// the block count.
inline bool tviews_info_consistent(const hgi_tviews_info &i)
{
    if (i.magic != HGI_TVIEWS_MAGIC) return false;
    if (i.plan_bytes != views_blob_bytes(i.count) || i.records_offset != views_records_offset() ||
        i.edge_prefix_offset != views_epre_offset(i.count) || i.interior_prefix_offset != views_ipre_offset(i.count))
        return false;
    if (i.count == 0)
        return i.edge_tiles == 0 && i.interior_tiles == 0 && i.max_width == 0 && (i.elem_size == 0 || i.elem_size == 2 || i.elem_size == 4);
    if (i.elem_size != 2 && i.elem_size != 4) return false;
    const uint64_t tiles = (uint64_t)i.edge_tiles + i.interior_tiles;
    return i.max_width != 0 && tiles >= i.count && list_blocks(i.edge_tiles, i.interior_tiles) + 8 < (1ull << 31);
}

enum TViewsVerdict {
    kTViewsOk = 0,
    // HGI_EINVAL
    kTViewsNullEntry, kTViewsSrcAlign, kTViewsSrcPitchAlign, kTViewsSrcPitch, kTViewsDstPitch, kTViewsTiles, kTViewsOutOut, kTViewsOutIn,
    // HGI_EUNSUPPORTED
    kTViewsFits32, kTViewsTail,
};

struct TViewsJudged {
    TViewsVerdict verdict;
    size_t a, b;                  // the list index the verdict names; for an aliasing pair the grid first, then the other view
    bool mixed_pitch;             // an aliasing pair that was refused without being judged: spans meet, pitches differ
};

// ---- the plan ----------------------------------------------------------------------------------------------------------------
// Every rule of a list in the order of include/hgi_tviews.h.  views != nullptr or n == 0; elem is 2 or 4 (or, with n == 0,
// 0); the entry point has judged the NULL arguments, plan_bytes >= views_blob_bytes(n) and elem.  On kTViewsOk the blob is
// written to h_plan and *info filled; otherwise neither is touched.  Nothing is allocated before the tile count is known to fit.
inline TViewsJudged tviews_plan(const hgi_tview_pair *views, size_t n, uint32_t elem, void *h_plan, hgi_tviews_info *info)
{
    TViewsJudged j = {kTViewsOk, 0, 0, false};
    auto refuse = [&](TViewsVerdict v, size_t a) {
        j.verdict = v;
        j.a = j.b = a;
        return j;
    };
    uint64_t tiles = 0, count = 0;
    bool too_many = false;
    for (size_t i = 0; i < n; ++i) {
        const hgi_tview_pair &v = views[i];
        if (v.width == 0 || v.height == 0) continue;
        if (!v.src || !v.dst) return refuse(kTViewsNullEntry, i);
        if (v.src % elem) return refuse(kTViewsSrcAlign, i);
        if (v.height > 1 && v.src_pitch % elem) return refuse(kTViewsSrcPitchAlign, i);
        if (v.height > 1 && v.src_pitch < (uint64_t)v.width * elem) return refuse(kTViewsSrcPitch, i);
        if (v.height > 1 && v.dst_pitch < v.width) return refuse(kTViewsDstPitch, i);
        ++count;
        if (!too_many) tiles += list_tiles(v.width, v.height);      // (a frame has fewer than 2^52 tiles: no wrap below 2^31 frames' worth)
        too_many = too_many || list_blocks(tiles, 0) + 8 >= (1ull << 31);
    }
    if (too_many) return refuse(kTViewsTiles, 0);
    if (count) {
        std::vector<MViewRect> rects;
        rects.reserve(2 * (size_t)count);
        for (size_t i = 0; i < n; ++i) {
            const hgi_tview_pair &v = views[i];
            if (v.width == 0 || v.height == 0) continue;
            rects.push_back(mview_rect(v.src, (uint64_t)v.width * elem, v.height, v.src_pitch, i, false));
            rects.push_back(mview_rect(v.dst, v.width, v.height, v.dst_pitch, i, true));
        }
        const MViewsJudged m = mviews_aliasing(rects);
        if (m.verdict != kMViewsOk) {
            j.verdict = m.verdict == kMViewsOutOut ? kTViewsOutOut : kTViewsOutIn;
            j.a = m.a;
            j.b = m.b;
            j.mixed_pitch = m.mixed_pitch;
            return j;
        }
    }
    for (size_t i = 0; i < n; ++i) {
        const hgi_tview_pair &v = views[i];
        if (v.width == 0 || v.height == 0) continue;
        const TypedJudged t = tview_typed_plan(v, elem);
        if (!t.fits32) return refuse(kTViewsFits32, i);
        if (!t.tail_ok) return refuse(kTViewsTail, i);
    }
    // every rule holds: the blob
    hgi_tviews_info o;
    memset(&o, 0, sizeof(o));
    o.magic = HGI_TVIEWS_MAGIC;
    o.count = (uint32_t)count;
    o.elem_size = elem;
    o.plan_bytes = views_blob_bytes(count);
    o.records_offset = views_records_offset();
    o.edge_prefix_offset = views_epre_offset(count);
    o.interior_prefix_offset = views_ipre_offset(count);
    if (count) {
        uint8_t *blob = static_cast<uint8_t *>(h_plan);
        memset(blob, 0, (size_t)o.plan_bytes);
        uint32_t m = 0, ne = 0, ni = 0, wmax = 0;
        for (size_t i = 0; i < n; ++i) {
            const hgi_tview_pair &v = views[i];
            if (v.width == 0 || v.height == 0) continue;
            const TypedPlan t = tview_typed_plan(v, elem).plan;
            const ViewFrame f = tview_frame(v, t);
            memcpy(blob + o.records_offset + 64 * (uint64_t)m, &f, 64);
            memcpy(blob + o.edge_prefix_offset + 4 * (uint64_t)m, &ne, 4);
            memcpy(blob + o.interior_prefix_offset + 4 * (uint64_t)m, &ni, 4);
            ne += t.p.epf;
            ni += t.p.ipf;
            wmax = v.width > wmax ? v.width : wmax;
            ++m;
        }
        o.edge_tiles = ne;
        o.interior_tiles = ni;
        o.max_width = wmax;
    }
    *info = o;
    return j;
}

}  // namespace hgi
