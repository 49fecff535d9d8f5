// View lists (hgi_views_plan / hgi_views_encode_dev / hgi_views_decode_dev, include/hgi_views.h): the host plan of one launch
// over the 128 x 64 tiles of many frames that each bring a shape, a read pitch and a write pitch of their own.  Two things the
// codec already has, put together:
//   * per frame, the geometry of a PITCHED call of a batch of one (csrc/hgi_pitched.h, pitched_plan): which tiles are interior,
//     the 32-bit pitches, the records of the two descriptors -- field by field;
//   * over the list, the launch order and the block -> tile map of the FRAME LISTS (csrc/hgi_framelist.h): every frame's ragged
//     tiles first, padded to a multiple of eight, then all interior tiles frame-major and row-major in contiguous eighths;
//     list_role / list_find / list_blocks / list_range_first run unchanged, view_tile is list_tile on this record.
// On top: the rules of a list (every one decided here, the HGI_EINVAL ones first) and the aliasing test on rectangles of bytes.
// The bound of a side and the page rule are companion/hgi_sides.h's.  The plan is written into a position-independent blob:
// records, then the two exclusive prefix arrays, addressed by the offsets of hgi_views_info.
// Plain C++: tests/cpp/test_views_plan.cpp runs it with g++.
//
// This library has no byte-checked path: a list with an entry that does not take the 32-bit buffer path is refused
// (HGI_EUNSUPPORTED) and the caller composes one pitched call per view.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/hgi_views.h"
#include "../companion/hgi_sides.h"
#include "../csrc/hgi_framelist.h"

namespace hgi {

static_assert(kListTileW == kPitchedTileW && kListTileH == kPitchedTileH, "one tile lattice for the map and the geometry");

// One non-empty frame of a launch (64 bytes: four scalar 16-byte loads).  tiles_x / tiles_y are not stored: view_tiles_x / _y.
struct ViewFrame {
    uint64_t src, dst;            // the frame's input and output (device addresses)
    uint32_t width, height;
    uint32_t full_x, full_y;      // tiles whose body lies inside the image (0 x 0: every tile is ragged)
    uint32_t sp32, dp32;          // read and write pitch (a one-row frame's: its width)
    uint32_t srec, drec;          // num_records of the read (span + tail) and write (span) descriptors
    FastDiv fd_fx;                // division by full_x (interior tiles, row-major)
};
static_assert(sizeof(ViewFrame) == 64, "one 64-byte record per frame");

// What a launch reads (kernel argument, by value): the three arrays of the device blob; `count` non-empty frames.
struct ViewArgs {
    const ViewFrame *frames;
    const uint32_t *epre, *ipre;
    uint32_t count, nedge, nint;
};

HGI_HD inline uint32_t view_tiles_x(uint32_t w) { return (uint32_t)(((uint64_t)w + kListTileW - 1) / kListTileW); }
HGI_HD inline uint32_t view_tiles_y(uint32_t h) { return (uint32_t)(((uint64_t)h + kListTileH - 1) / kListTileH); }

// ---- the blob ---------------------------------------------------------------------------------------------------------------
inline uint64_t views_prefix_bytes(uint64_t count) { return (4 * count + 15u) & ~(uint64_t)15u; }
inline uint64_t views_records_offset() { return 0; }
inline uint64_t views_epre_offset(uint64_t count) { return 64 * count; }
inline uint64_t views_ipre_offset(uint64_t count) { return 64 * count + views_prefix_bytes(count); }
inline uint64_t views_blob_bytes(uint64_t count) { return 64 * count + 2 * views_prefix_bytes(count); }

// ---- per-frame geometry: pitched_plan of a batch of one ------------------------------------------------------------------------
inline PitchedPlan view_pitched_plan(const hgi_view_pair &v)
{
    const PitchedFrames pf = {v.width, v.height, 1u, v.src_pitch, v.dst_pitch, 0, 0};
    return pitched_plan(v.src, pf, false);
}

inline ViewFrame view_frame(const hgi_view_pair &v, const PitchedPlan &p)
{
    ViewFrame f;
    f.src = v.src;
    f.dst = v.dst;
    f.width = v.width;
    f.height = v.height;
    f.full_x = p.ix;
    f.full_y = p.iy;
    f.sp32 = p.sp32;
    f.dp32 = p.dp32;
    f.srec = p.srec;
    f.drec = p.drec;
    f.fd_fx = p.fd_ix;
    return f;
}

// ---- the map: list_tile on this record ---------------------------------------------------------------------------------------
HGI_HD inline void view_tile(ListBlock &r, const ViewFrame &F, uint32_t first)
{
    uint32_t i = r.t - first;
    if (r.edge) {
        const uint32_t tx = view_tiles_x(F.width), ty = view_tiles_y(F.height);
        const uint32_t wr = tx - F.full_x, right = wr * ty;
        if (i < right) {
            r.ty = i / wr;
            r.tx = F.full_x + (i - r.ty * wr);
        } else {
            i -= right;
            r.ty = F.full_y + i / F.full_x;
            r.tx = i % F.full_x;
        }
    } else {
        r.ty = fdiv(i, F.fd_fx);
        r.tx = i - r.ty * F.full_x;
    }
}

// The whole map, as the host test walks it (the kernels run list_role / list_find / view_tile with their loads placed early).
inline ListBlock view_block(uint32_t b, const ViewArgs &a)
{
    ListBlock r = list_role(b, a.nedge, a.nint);
    if (r.idle || a.count == 0) return r;
    const uint32_t *pre = r.edge ? a.epre : a.ipre;
    r.frame = list_find(pre, a.count, r.t);
    view_tile(r, a.frames[r.frame], pre[r.frame]);
    return r;
}

// The three arrays of a blob that lies at `base` (host: the caller's memory; launch: the device address), per `info`.
inline ViewArgs view_args(const void *base, const hgi_views_info &info)
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

// What a launch checks of the host struct it is handed: the magic, the sizes and offsets against the count, the block count.
inline bool views_info_consistent(const hgi_views_info &i)
{
    if (i.magic != HGI_VIEWS_MAGIC || i.reserved != 0) return false;
    if (i.plan_bytes != views_blob_bytes(i.count) || i.records_offset != views_records_offset() ||
        i.edge_prefix_offset != views_epre_offset(i.count) || i.interior_prefix_offset != views_ipre_offset(i.count))
        return false;
    if (i.count == 0) return i.edge_tiles == 0 && i.interior_tiles == 0 && i.max_width == 0;
    const uint64_t tiles = (uint64_t)i.edge_tiles + i.interior_tiles;
    return i.max_width != 0 && tiles >= i.count && list_blocks(i.edge_tiles, i.interior_tiles) + 8 < (1ull << 31);
}

// ---- aliasing: rectangles of bytes ---------------------------------------------------------------------------------------------
typedef unsigned __int128 views_u128;

// One side of one entry: `width` bytes on each of `height` rows `pitch` apart (a one-row frame's pitch counts as its width).
struct ViewRect {
    views_u128 lo, hi;            // the byte span [lo, hi)
    uint64_t pitch;
    uint32_t width, height;
    size_t index;                 // list index
    bool out;
};

inline ViewRect view_rect(uint64_t p, uint32_t w, uint32_t h, uint64_t pitch, size_t index, bool out)
{
    ViewRect r;
    r.pitch = h > 1 ? pitch : w;
    r.lo = p;
    r.hi = (views_u128)p + (views_u128)(h - 1) * r.pitch + w;
    r.width = w;
    r.height = h;
    r.index = index;
    r.out = out;
    return r;
}

// Two rectangles whose spans meet.  0: disjoint; 1: they share a byte; 2: different pitches (not judged: refused).  With the
// lower address as origin and the common pitch P, the other one starts at column d % P of row d / P; one that runs over the
// end of a row of that lattice wraps into the rows the first one holds (their spans meet), so it shares a byte with it.
// A one-row view is an interval of bytes and has no pitch to differ by: it shares a byte with the other view iff the first row
// of that one which ends behind the interval's start begins in front of its end.
inline bool view_row_meets(const ViewRect &row, const ViewRect &r)
{
    const views_u128 k = row.lo < r.lo + r.width ? 0 : (row.lo - r.lo - r.width) / r.pitch + 1;
    return k < r.height && r.lo + k * r.pitch < row.hi;
}

inline int view_rects_meet(const ViewRect &x, const ViewRect &y)
{
    if (x.height == 1) return view_row_meets(x, y) ? 1 : 0;
    if (y.height == 1) return view_row_meets(y, x) ? 1 : 0;
    if (x.pitch != y.pitch) return 2;
    const ViewRect &a = x.lo <= y.lo ? x : y, &b = x.lo <= y.lo ? y : x;
    const views_u128 d = b.lo - a.lo, P = a.pitch;
    const views_u128 col = d % P, row = d / P;
    if (col + b.width > P) return 1;
    return col >= a.width || row >= a.height ? 0 : 1;
}

enum ViewsVerdict {
    kViewsOk = 0,
    // HGI_EINVAL
    kViewsNullEntry, kViewsSrcPitch, kViewsDstPitch, kViewsTiles, kViewsOutOut, kViewsOutIn,
    // HGI_EUNSUPPORTED
    kViewsFits32, kViewsTail,
};

struct ViewsJudged {
    ViewsVerdict verdict;
    size_t a, b;                  // the list index the verdict names; for an aliasing pair the output first, then the other view
    bool mixed_pitch;             // an aliasing pair that was refused without being judged: spans meet, pitches differ
};

// list_overlap's sorted sweep, carried on to every pair whose spans meet and of which one is an output: the spans in the order
// of their first byte; behind each start, the earlier spans that reach past it are the ones it meets.  Two lists of such
// earlier spans are kept, outputs and inputs; an input is tested against the outputs only, so inputs that overlap each other
// cost nothing.  A span that no longer reaches the sweep's position is dropped when a scan passes it: O(n log n + pairs met).
inline ViewsJudged views_aliasing(std::vector<ViewRect> &rects)
{
    std::sort(rects.begin(), rects.end(), [](const ViewRect &x, const ViewRect &y) { return x.lo != y.lo ? x.lo < y.lo : x.index < y.index; });
    std::vector<const ViewRect *> outs, ins;
    // the first offending pair of each kind, in the order of the sweep: two outputs are reported before an output and an input
    ViewsJudged oo = {kViewsOk, 0, 0, false}, oi = {kViewsOk, 0, 0, false};
    auto scan = [&](std::vector<const ViewRect *> &live, const ViewRect &s) {
        size_t keep = 0;
        for (size_t i = 0; i < live.size(); ++i) {
            const ViewRect *e = live[i];
            if (e->hi <= s.lo) continue;      // (sorted by lo: it meets nothing that follows either)
            live[keep++] = e;
            ViewsJudged &j = e->out && s.out ? oo : oi;
            if (j.verdict != kViewsOk) continue;
            const int m = view_rects_meet(*e, s);
            if (m == 0) continue;
            j.verdict = e->out && s.out ? kViewsOutOut : kViewsOutIn;
            j.a = e->out ? e->index : s.index;
            j.b = e->out ? s.index : e->index;
            if (e->out && s.out && j.b < j.a) std::swap(j.a, j.b);
            j.mixed_pitch = m == 2;
        }
        live.resize(keep);
    };
    for (const ViewRect &s : rects) {
        if (oo.verdict != kViewsOk) break;
        scan(outs, s);
        if (s.out) scan(ins, s);
        (s.out ? outs : ins).push_back(&s);
    }
    return oo.verdict != kViewsOk ? oo : oi;
}

// ---- the plan ----------------------------------------------------------------------------------------------------------------
// Every rule of a list in the order of include/hgi_views.h.  views != nullptr or n == 0; the entry point has judged the NULL
// arguments and plan_bytes >= views_blob_bytes(n).  On kViewsOk the blob is written to h_plan and *info filled; otherwise
// neither is touched.  Nothing is allocated before the tile count is known to fit.
inline ViewsJudged views_plan(const hgi_view_pair *views, size_t n, void *h_plan, hgi_views_info *info)
{
    ViewsJudged j = {kViewsOk, 0, 0, false};
    auto refuse = [&](ViewsVerdict v, size_t a) {
        j.verdict = v;
        j.a = j.b = a;
        return j;
    };
    uint64_t tiles = 0, count = 0;
    bool too_many = false;
    for (size_t i = 0; i < n; ++i) {
        const hgi_view_pair &v = views[i];
        if (v.width == 0 || v.height == 0) continue;
        if (!v.src || !v.dst) return refuse(kViewsNullEntry, i);
        if (v.height > 1 && v.src_pitch < v.width) return refuse(kViewsSrcPitch, i);
        if (v.height > 1 && v.dst_pitch < v.width) return refuse(kViewsDstPitch, i);
        ++count;
        if (!too_many) tiles += list_tiles(v.width, v.height);      // (a frame has fewer than 2^52 tiles: no wrap below 2^31 frames' worth)
        too_many = too_many || list_blocks(tiles, 0) + 8 >= (1ull << 31);
    }
    if (too_many) return refuse(kViewsTiles, 0);
    if (count) {
        std::vector<ViewRect> rects;
        rects.reserve(2 * (size_t)count);
        for (size_t i = 0; i < n; ++i) {
            const hgi_view_pair &v = views[i];
            if (v.width == 0 || v.height == 0) continue;
            rects.push_back(view_rect(v.src, v.width, v.height, v.src_pitch, i, false));
            rects.push_back(view_rect(v.dst, v.width, v.height, v.dst_pitch, i, true));
        }
        j = views_aliasing(rects);
        if (j.verdict != kViewsOk) return j;
    }
    for (size_t i = 0; i < n; ++i) {
        const hgi_view_pair &v = views[i];
        if (v.width == 0 || v.height == 0) continue;
        const uint64_t sp = v.height > 1 ? v.src_pitch : v.width, dp = v.height > 1 ? v.dst_pitch : v.width;
        if (!side_fits32(v.height, sp > dp ? sp : dp)) return refuse(kViewsFits32, i);
        if (v.width % 4 != 0 && !tail_in_page(v.src, v.width, v.height, v.src_pitch, 0, 1, 3)) return refuse(kViewsTail, i);
    }
    // every rule holds: the blob
    hgi_views_info o;
    memset(&o, 0, sizeof(o));
    o.magic = HGI_VIEWS_MAGIC;
    o.count = (uint32_t)count;
    o.plan_bytes = views_blob_bytes(count);
    o.records_offset = views_records_offset();
    o.edge_prefix_offset = views_epre_offset(count);
    o.interior_prefix_offset = views_ipre_offset(count);
    if (count) {
        uint8_t *blob = static_cast<uint8_t *>(h_plan);
        memset(blob, 0, (size_t)o.plan_bytes);
        uint32_t m = 0, ne = 0, ni = 0, wmax = 0;
        for (size_t i = 0; i < n; ++i) {
            const hgi_view_pair &v = views[i];
            if (v.width == 0 || v.height == 0) continue;
            const PitchedPlan p = view_pitched_plan(v);
            const ViewFrame f = view_frame(v, p);
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
    }
    *info = o;
    return j;
}

}  // namespace hgi
