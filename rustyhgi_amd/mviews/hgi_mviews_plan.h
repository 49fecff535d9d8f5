// Mapped view lists (hgi_mviews_plan / hgi_mviews_decode_dev, include/hgi_mviews.h): the host plan of one launch over the
// 128 x 64 tiles of many grids that each bring a shape, a read pitch and -- for the frame of E-byte elements that is written --
// a BYTE pitch of their own.  It is the view lists' plan (../views/hgi_views_plan.h) with the written side in bytes:
//   * the record is that plan's 64-byte ViewFrame, the read side field by field pitched_plan's of a batch of one; on the written
//     side dp32 is the byte pitch and drec the span (h - 1) * pitch + w * E, as in map_plan (../map/hgi_map_plan.h);
//   * the blob, the launch order, the block -> tile map and the frame search are the view lists' unchanged (view_block,
//     views_blob_bytes, the offsets);
//   * the rules of a list are the view lists' plus those of E-byte elements; the aliasing test is that plan's sweep on rectangles
//     of bytes with output rectangles w * E bytes wide (a row of 2^30 pixels and more does not fit ViewRect's 32-bit width: the
//     rectangle here carries 64 bits and the sweep is written once more for it).
// On top: the bounding byte interval of all output spans, which the launch tests the table against.
// Plain C++: tests/cpp/test_mviews_plan.cpp runs it with g++.
//
// This library has no byte-checked path: a list with an entry that does not take the 32-bit buffer path is refused
// (HGI_EUNSUPPORTED) and the caller composes one mapped decode per view.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/hgi_mviews.h"
#include "../views/hgi_views_plan.h"

namespace hgi {

// ---- per-frame geometry: pitched_plan of a batch of one on the grid side, the written side in bytes --------------------------
inline PitchedPlan mview_pitched_plan(const hgi_mview_pair &v)
{
    const PitchedFrames pf = {v.width, v.height, 1u, v.src_pitch, v.src_pitch, 0, 0};
    return pitched_plan(v.src, pf, false);
}

// The output's pitch (a one-row frame's counts as its row) and span, bytes.
inline uint64_t mview_out_pitch(const hgi_mview_pair &v, uint32_t elem) { return v.height > 1 ? v.dst_pitch : (uint64_t)v.width * elem; }
inline uint64_t mview_out_span(const hgi_mview_pair &v, uint32_t elem) { return side_span((uint64_t)v.width * elem, v.height, mview_out_pitch(v, elem)); }

// `p`: mview_pitched_plan(v) of an entry that passed every rule (both sides fit 32 bits).
inline ViewFrame mview_frame(const hgi_mview_pair &v, const PitchedPlan &p, uint32_t elem)
{
    const hgi_view_pair u = {v.src, v.dst, v.width, v.height, v.src_pitch, v.dst_pitch};
    ViewFrame f = view_frame(u, p);
    f.dp32 = (uint32_t)mview_out_pitch(v, elem);
    f.drec = (uint32_t)mview_out_span(v, elem);
    return f;
}

// The three arrays of a blob that lies at `base`, per `info` (view_args on this library's struct).
inline ViewArgs mview_args(const void *base, const hgi_mviews_info &info)
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
// the block count, the output interval.
inline bool mviews_info_consistent(const hgi_mviews_info &i)
{
    if (i.magic != HGI_MVIEWS_MAGIC) return false;
    if (i.plan_bytes != views_blob_bytes(i.count) || i.records_offset != views_records_offset() ||
        i.edge_prefix_offset != views_epre_offset(i.count) || i.interior_prefix_offset != views_ipre_offset(i.count))
        return false;
    if (i.count == 0)
        return i.edge_tiles == 0 && i.interior_tiles == 0 && i.max_width == 0 && i.dst_lo == 0 && i.dst_hi == 0 &&
               (i.elem_size == 0 || i.elem_size == 2 || i.elem_size == 4);
    if (i.elem_size != 2 && i.elem_size != 4) return false;
    const uint64_t tiles = (uint64_t)i.edge_tiles + i.interior_tiles;
    return i.max_width != 0 && tiles >= i.count && list_blocks(i.edge_tiles, i.interior_tiles) + 8 < (1ull << 31) && i.dst_lo != 0 &&
           i.dst_lo % i.elem_size == 0 && i.dst_hi >= i.dst_lo + (uint64_t)i.max_width * i.elem_size;
}

// ---- aliasing: rectangles of bytes, rows of up to 2^34 bytes ---------------------------------------------------------------------
// ViewRect and its three functions of ../views/hgi_views_plan.h with a 64-bit row: the same tests, the same sweep, the same order
// of reports.
struct MViewRect {
    views_u128 lo, hi;            // the byte span [lo, hi)
    uint64_t pitch, width;        // bytes between rows (a one-row frame's: its row), bytes of a row
    uint32_t height;
    size_t index;                 // list index
    bool out;
};

inline MViewRect mview_rect(uint64_t p, uint64_t row_bytes, uint32_t h, uint64_t pitch, size_t index, bool out)
{
    MViewRect r;
    r.pitch = h > 1 ? pitch : row_bytes;
    r.lo = p;
    r.hi = (views_u128)p + (views_u128)(h - 1) * r.pitch + row_bytes;
    r.width = row_bytes;
    r.height = h;
    r.index = index;
    r.out = out;
    return r;
}

inline bool mview_row_meets(const MViewRect &row, const MViewRect &r)
{
    const views_u128 k = row.lo < r.lo + r.width ? 0 : (row.lo - r.lo - r.width) / r.pitch + 1;
    return k < r.height && r.lo + k * r.pitch < row.hi;
}

// 0: disjoint; 1: they share a byte; 2: different pitches (not judged: refused)
inline int mview_rects_meet(const MViewRect &x, const MViewRect &y)
{
    if (x.height == 1) return mview_row_meets(x, y) ? 1 : 0;
    if (y.height == 1) return mview_row_meets(y, x) ? 1 : 0;
    if (x.pitch != y.pitch) return 2;
    const MViewRect &a = x.lo <= y.lo ? x : y, &b = x.lo <= y.lo ? y : x;
    const views_u128 d = b.lo - a.lo, P = a.pitch;
    const views_u128 col = d % P, row = d / P;
    if (col + b.width > P) return 1;
    return col >= a.width || row >= a.height ? 0 : 1;
}

enum MViewsVerdict {
    kMViewsOk = 0,
    // HGI_EINVAL
    kMViewsNullEntry, kMViewsSrcPitch, kMViewsDstAlign, kMViewsDstPitchAlign, kMViewsDstPitch, kMViewsTiles, kMViewsOutOut, kMViewsOutIn,
    // HGI_EUNSUPPORTED
    kMViewsFits32, kMViewsTail,
};

struct MViewsJudged {
    MViewsVerdict verdict;
    size_t a, b;                  // the list index the verdict names; for an aliasing pair the output first, then the other view
    bool mixed_pitch;             // an aliasing pair that was refused without being judged: spans meet, pitches differ
};

// views_aliasing's sweep: the spans in the order of their first byte; behind each start, the earlier spans that reach past it
// are the ones it meets.  An input is tested against the outputs only.  O(n log n + pairs met).
inline MViewsJudged mviews_aliasing(std::vector<MViewRect> &rects)
{
    std::sort(rects.begin(), rects.end(), [](const MViewRect &x, const MViewRect &y) { return x.lo != y.lo ? x.lo < y.lo : x.index < y.index; });
    std::vector<const MViewRect *> outs, ins;
    // the first offending pair of each kind, in the order of the sweep: two outputs are reported before an output and an input
    MViewsJudged oo = {kMViewsOk, 0, 0, false}, oi = {kMViewsOk, 0, 0, false};
    auto scan = [&](std::vector<const MViewRect *> &live, const MViewRect &s) {
        size_t keep = 0;
        for (size_t i = 0; i < live.size(); ++i) {
            const MViewRect *e = live[i];
            if (e->hi <= s.lo) continue;      // (sorted by lo: it meets nothing that follows either)
            live[keep++] = e;
            MViewsJudged &j = e->out && s.out ? oo : oi;
            if (j.verdict != kMViewsOk) continue;
            const int m = mview_rects_meet(*e, s);
            if (m == 0) continue;
            j.verdict = e->out && s.out ? kMViewsOutOut : kMViewsOutIn;
            j.a = e->out ? e->index : s.index;
            j.b = e->out ? s.index : e->index;
            if (e->out && s.out && j.b < j.a) std::swap(j.a, j.b);
            j.mixed_pitch = m == 2;
        }
        live.resize(keep);
    };
    for (const MViewRect &s : rects) {
        if (oo.verdict != kMViewsOk) break;
        scan(outs, s);
        if (s.out) scan(ins, s);
        (s.out ? outs : ins).push_back(&s);
    }
    return oo.verdict != kMViewsOk ? oo : oi;
}

// ---- the plan ----------------------------------------------------------------------------------------------------------------
// Every rule of a list in the order of include/hgi_mviews.h.  views != nullptr or n == 0; elem is 2 or 4; the entry point has
// judged the NULL arguments, plan_bytes >= views_blob_bytes(n) and elem.  On kMViewsOk the blob is written to h_plan and *info
// filled; otherwise neither is touched.  Nothing is allocated before the tile count is known to fit.
inline MViewsJudged mviews_plan(const hgi_mview_pair *views, size_t n, uint32_t elem, void *h_plan, hgi_mviews_info *info)
{
    MViewsJudged j = {kMViewsOk, 0, 0, false};
    auto refuse = [&](MViewsVerdict v, size_t a) {
        j.verdict = v;
        j.a = j.b = a;
        return j;
    };
    uint64_t tiles = 0, count = 0;
    bool too_many = false;
    for (size_t i = 0; i < n; ++i) {
        const hgi_mview_pair &v = views[i];
        if (v.width == 0 || v.height == 0) continue;
        if (!v.src || !v.dst) return refuse(kMViewsNullEntry, i);
        if (v.height > 1 && v.src_pitch < v.width) return refuse(kMViewsSrcPitch, i);
        if (v.dst % elem) return refuse(kMViewsDstAlign, i);
        if (v.height > 1 && v.dst_pitch % elem) return refuse(kMViewsDstPitchAlign, i);
        if (v.height > 1 && v.dst_pitch < (uint64_t)v.width * elem) return refuse(kMViewsDstPitch, i);
        ++count;
        if (!too_many) tiles += list_tiles(v.width, v.height);      // (a frame has fewer than 2^52 tiles: no wrap below 2^31 frames' worth)
        too_many = too_many || list_blocks(tiles, 0) + 8 >= (1ull << 31);
    }
    if (too_many) return refuse(kMViewsTiles, 0);
    views_u128 lo = 0, hi = 0;
    if (count) {
        std::vector<MViewRect> rects;
        rects.reserve(2 * (size_t)count);
        bool first = true;
        for (size_t i = 0; i < n; ++i) {
            const hgi_mview_pair &v = views[i];
            if (v.width == 0 || v.height == 0) continue;
            rects.push_back(mview_rect(v.src, v.width, v.height, v.src_pitch, i, false));
            rects.push_back(mview_rect(v.dst, (uint64_t)v.width * elem, v.height, v.dst_pitch, i, true));
            const MViewRect &o = rects.back();
            lo = first || o.lo < lo ? o.lo : lo;
            hi = first || o.hi > hi ? o.hi : hi;
            first = false;
        }
        j = mviews_aliasing(rects);
        if (j.verdict != kMViewsOk) return j;
    }
    for (size_t i = 0; i < n; ++i) {
        const hgi_mview_pair &v = views[i];
        if (v.width == 0 || v.height == 0) continue;
        const uint64_t sp = v.height > 1 ? v.src_pitch : v.width, dp = mview_out_pitch(v, elem);
        if (!side_fits32(v.height, sp > dp ? sp : dp)) return refuse(kMViewsFits32, i);
        if (v.width % 4 != 0 && !tail_in_page(v.src, v.width, v.height, v.src_pitch, 0, 1, 3)) return refuse(kMViewsTail, i);
    }
    // every rule holds: the blob
    hgi_mviews_info o;
    memset(&o, 0, sizeof(o));
    o.magic = HGI_MVIEWS_MAGIC;
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
            const hgi_mview_pair &v = views[i];
            if (v.width == 0 || v.height == 0) continue;
            const PitchedPlan p = mview_pitched_plan(v);
            const ViewFrame f = mview_frame(v, p, elem);
            memcpy(blob + o.records_offset + 64 * (uint64_t)m, &f, 64);
            memcpy(blob + o.edge_prefix_offset + 4 * (uint64_t)m, &ne, 4);
            memcpy(blob + o.interior_prefix_offset + 4 * (uint64_t)m, &ni, 4);
            ne += p.epf;
            ni += p.ipf;
            wmax = v.width > wmax ? v.width : wmax;
            ++m;
        }
        o.edge_tiles = ne;
        o.interior_tiles = ni;
        o.max_width = wmax;
        // (an output span that ends behind the last address is clipped to it: nothing lies there that a table could meet)
        o.dst_lo = (uint64_t)lo;
        o.dst_hi = hi > (views_u128)UINT64_MAX ? UINT64_MAX : (uint64_t)hi;
    }
    *info = o;
    return j;
}

}  // namespace hgi
