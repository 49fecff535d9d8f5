// Scaled view lists (hgi_sviews_plan / hgi_sviews_decode_dev, include/hgi_sviews.h): the host plan of one launch over the
// 128 x 64 tiles of the 1 / 2^s images of many stored grids that each bring a shape, a read pitch and a write pitch of their own,
// and the launch's whole judgement.  It is the view lists' plan (../views/hgi_views_plan.h) on the view the scaled decoder
// decodes (../csrc/hgi_fused_scaled.hip, launch_decode_scaled):
//   * the record is that plan's 64-byte ViewFrame and holds the VIEW: width / height are sw x sh = ceil(w / 2^s) x ceil(h / 2^s),
//     sp32 the view's row pitch src_pitch << s, srec the grid's span, dp32 / drec the output's pitch and span, full_x / full_y
//     the interior tiles as launch_decode_scaled computes ix / iy with frame_bytes = the span -- its last-row rule included, at
//     the deepest halo a launch of this library stages (five levels: the plan does not know the depth);
//   * the blob, the launch order, the block -> tile map and the frame search are the view lists' unchanged (view_block,
//     views_blob_bytes, the offsets; view_ctx and views_tile_launch on the device side);
//   * the aliasing test is that plan's sweep (views_aliasing) on the whole grid as the input rectangle and the sw x sh image as
//     the output rectangle.
// The descriptor of the read side ranges over the span and nothing is added to it: this library has no page rule.
// Plain C++, no HIP: tests/cpp/test_sviews_plan.cpp runs it with g++.
//
// This library has no byte-checked path: a list with an entry that does not take the 32-bit buffer path is refused
// (HGI_EUNSUPPORTED) and the caller composes one scaled decode per view.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/hgi_sviews.h"
#include "../views/hgi_views_plan.h"

namespace hgi {

constexpr uint32_t kSViewsMaxTileLevels = 5;      // r <= 5 runs in the tile (split_levels): the deepest halo a launch stages

// ---- per-grid geometry: the view of launch_decode_scaled -------------------------------------------------------------------
struct SViewGeom {
    uint32_t sw, sh;              // the output image
    uint64_t span, rp;            // the grid's byte span; the view's row pitch (sh == 1: the span -- rows below read zeros)
    uint64_t dp, dspan;           // the output's pitch (a one-row image's: its row) and span
    bool read32, write32;         // the two sides take the 32-bit buffer path
    uint32_t ix, iy;              // interior tiles (0 x 0: every tile is ragged); valid where both sides fit
};

inline uint32_t sview_dim(uint32_t v, uint32_t s) { return (uint32_t)((((uint64_t)v - 1) >> s) + 1); }      // ceil(v / 2^s), v >= 1

// v: a non-empty entry that passed the pitch rules; s <= 31.
inline SViewGeom sview_geom(const hgi_sview_pair &v, uint32_t s)
{
    SViewGeom g;
    g.sw = sview_dim(v.width, s);
    g.sh = sview_dim(v.height, s);
    const views_u128 span = (views_u128)(v.height - 1) * (v.height > 1 ? v.src_pitch : 0) + v.width;
    const views_u128 rp = g.sh > 1 ? (views_u128)v.src_pitch << s : span;
    const uint64_t tx = view_tiles_x(g.sw), ty = view_tiles_y(g.sh);
    // launch_decode_scaled's read32: every 32-bit offset the staging forms -- rows up to the last tile's halo, columns up to
    // its halo columns plus a chunk's 16 << s bytes
    const uint64_t rows_max = ty * kListTileH + 64, cols_max = (tx * kListTileW + 64 + 16) << s;
    g.read32 = span < (1ull << 32) && rp < (1ull << 32) && rows_max * (uint64_t)rp + cols_max + 64 < (1ull << 32);
    g.span = (uint64_t)span;      // (meaningful where read32)
    g.rp = (uint64_t)rp;
    g.dp = g.sh > 1 ? v.dst_pitch : g.sw;
    g.write32 = side_fits32(g.sh, g.dp);
    g.dspan = g.write32 ? side_span(g.sw, g.sh, g.dp) : 0;
    g.ix = g.sw / kListTileW;
    g.iy = g.sh / kListTileH;
    if (g.read32) {
        // launch_decode_scaled's last-row rule: a wide load reads 16 << s bytes for 16 view bytes; on the view's last row the
        // dword behind the row's last view byte can lie past the span, and the range check would drop it whole.  Interior
        // tiles then keep off that row, which a tile reads up to 64 + hoff(nh - 1) rows below its origin.
        const uint32_t reach = kListTileH + (2u << (kSViewsMaxTileLevels - 1));
        const bool hazard = (uint64_t)(g.sh - 1) * g.rp + (((uint64_t)g.ix * kListTileW) << s) > g.span;
        if (hazard)
            while (g.iy > 0 && (uint64_t)(g.iy - 1) * kListTileH + reach >= g.sh - 1) --g.iy;
    }
    if (g.ix == 0 || g.iy == 0) g.ix = g.iy = 0;
    return g;
}

// `g`: sview_geom(v, s) of an entry that passed every rule (both sides fit 32 bits).
inline ViewFrame sview_frame(const hgi_sview_pair &v, const SViewGeom &g)
{
    ViewFrame f;
    f.src = v.src;
    f.dst = v.dst;
    f.width = g.sw;
    f.height = g.sh;
    f.full_x = g.ix;
    f.full_y = g.iy;
    f.sp32 = (uint32_t)g.rp;
    f.dp32 = (uint32_t)g.dp;
    f.srec = (uint32_t)g.span;
    f.drec = (uint32_t)g.dspan;
    f.fd_fx = make_fastdiv(g.ix ? g.ix : 1u);
    return f;
}

// The three arrays of a blob that lies at `base`, per `info` (view_args on this library's struct).
inline ViewArgs sview_args(const void *base, const hgi_sviews_info &info)
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

// What a launch checks of the host struct it is handed: the magic, the shift, the sizes and offsets against the count, the block
// count.
inline bool sviews_info_consistent(const hgi_sviews_info &i)
{
    if (i.magic != HGI_SVIEWS_MAGIC || i.shift > 31) return false;
    if (i.plan_bytes != views_blob_bytes(i.count) || i.records_offset != views_records_offset() ||
        i.edge_prefix_offset != views_epre_offset(i.count) || i.interior_prefix_offset != views_ipre_offset(i.count))
        return false;
    if (i.count == 0) return i.edge_tiles == 0 && i.interior_tiles == 0 && i.max_width == 0;
    const uint64_t tiles = (uint64_t)i.edge_tiles + i.interior_tiles;
    return i.shift != 0 && i.max_width != 0 && tiles >= i.count && list_blocks(i.edge_tiles, i.interior_tiles) + 8 < (1ull << 31);
}

enum SViewsVerdict {
    kSViewsOk = 0,
    // HGI_EINVAL
    kSViewsNullEntry, kSViewsSrcPitch, kSViewsDstPitch, kSViewsTiles, kSViewsOutOut, kSViewsOutIn,
    // HGI_EUNSUPPORTED
    kSViewsShiftZero, kSViewsRead32, kSViewsWrite32,
};

struct SViewsJudged {
    SViewsVerdict verdict;
    size_t a, b;                  // the list index the verdict names; for an aliasing pair the output first, then the other view
    bool mixed_pitch;             // an aliasing pair that was refused without being judged: spans meet, pitches differ
};

// ---- the plan ----------------------------------------------------------------------------------------------------------------
// Every rule of a list in the order of include/hgi_sviews.h.  views != nullptr or n == 0; the entry point has judged the NULL
// arguments, plan_bytes >= views_blob_bytes(n) and shift <= 31.  On kSViewsOk the blob is written to h_plan and *info filled;
// otherwise neither is touched.  Nothing is allocated before the tile count is known to fit.
inline SViewsJudged sviews_plan(const hgi_sview_pair *views, size_t n, uint32_t shift, void *h_plan, hgi_sviews_info *info)
{
    SViewsJudged j = {kSViewsOk, 0, 0, false};
    auto refuse = [&](SViewsVerdict v, size_t a) {
        j.verdict = v;
        j.a = j.b = a;
        return j;
    };
    uint64_t tiles = 0, count = 0;
    bool too_many = false;
    for (size_t i = 0; i < n; ++i) {
        const hgi_sview_pair &v = views[i];
        if (v.width == 0 || v.height == 0) continue;
        if (!v.src || !v.dst) return refuse(kSViewsNullEntry, i);
        if (v.height > 1 && v.src_pitch < v.width) return refuse(kSViewsSrcPitch, i);
        const uint32_t sw = sview_dim(v.width, shift), sh = sview_dim(v.height, shift);
        if (sh > 1 && v.dst_pitch < sw) return refuse(kSViewsDstPitch, i);
        ++count;
        if (!too_many) tiles += list_tiles(sw, sh);      // (an image has fewer than 2^52 tiles: no wrap below 2^31 images' worth)
        too_many = too_many || list_blocks(tiles, 0) + 8 >= (1ull << 31);
    }
    if (too_many) return refuse(kSViewsTiles, 0);
    if (count) {
        std::vector<ViewRect> rects;
        rects.reserve(2 * (size_t)count);
        for (size_t i = 0; i < n; ++i) {
            const hgi_sview_pair &v = views[i];
            if (v.width == 0 || v.height == 0) continue;
            rects.push_back(view_rect(v.src, v.width, v.height, v.src_pitch, i, false));
            rects.push_back(view_rect(v.dst, sview_dim(v.width, shift), sview_dim(v.height, shift), v.dst_pitch, i, true));
        }
        const ViewsJudged a = views_aliasing(rects);
        if (a.verdict != kViewsOk) {
            j.verdict = a.verdict == kViewsOutOut ? kSViewsOutOut : kSViewsOutIn;
            j.a = a.a;
            j.b = a.b;
            j.mixed_pitch = a.mixed_pitch;
            return j;
        }
    }
    if (shift == 0 && count) return refuse(kSViewsShiftZero, 0);
    for (size_t i = 0; i < n; ++i) {
        const hgi_sview_pair &v = views[i];
        if (v.width == 0 || v.height == 0) continue;
        const SViewGeom g = sview_geom(v, shift);
        if (!g.read32) return refuse(kSViewsRead32, i);
        if (!g.write32) return refuse(kSViewsWrite32, i);
    }
    // every rule holds: the blob
    hgi_sviews_info o;
    memset(&o, 0, sizeof(o));
    o.magic = HGI_SVIEWS_MAGIC;
    o.count = (uint32_t)count;
    o.shift = shift;
    o.plan_bytes = views_blob_bytes(count);
    o.records_offset = views_records_offset();
    o.edge_prefix_offset = views_epre_offset(count);
    o.interior_prefix_offset = views_ipre_offset(count);
    if (count) {
        uint8_t *blob = static_cast<uint8_t *>(h_plan);
        memset(blob, 0, (size_t)o.plan_bytes);
        uint32_t m = 0, ne = 0, ni = 0, wmax = 0;
        for (size_t i = 0; i < n; ++i) {
            const hgi_sview_pair &v = views[i];
            if (v.width == 0 || v.height == 0) continue;
            const SViewGeom g = sview_geom(v, shift);
            const ViewFrame f = sview_frame(v, g);
            memcpy(blob + o.records_offset + 64 * (uint64_t)m, &f, 64);
            memcpy(blob + o.edge_prefix_offset + 4 * (uint64_t)m, &ne, 4);
            memcpy(blob + o.interior_prefix_offset + 4 * (uint64_t)m, &ni, 4);
            const uint32_t ipf = g.ix * g.iy;
            ne += (uint32_t)list_tiles(g.sw, g.sh) - ipf;
            ni += ipf;
            wmax = g.sw > wmax ? g.sw : wmax;
            ++m;
        }
        o.edge_tiles = ne;
        o.interior_tiles = ni;
        o.max_width = wmax;
    }
    *info = o;
    return j;
}

// ---- the launch's judgement --------------------------------------------------------------------------------------------------
enum SViewsLaunchVerdict {
    kSViewsLaunch = 0,            // every rule holds: k / up are set
    kSViewsEmpty,                 // a plan of no grid: HGI_OK, nothing launched
    // HGI_EINVAL
    kSViewsInfoNull, kSViewsInfo, kSViewsPlanNull, kSViewsPlanAlign, kSViewsLevelsRange, kSViewsInterp,
    // HGI_EUNSUPPORTED
    kSViewsLevelsZero, kSViewsGather, kSViewsDepth,
};

struct SViewsLaunchJudged {
    hgi_status status;
    SViewsLaunchVerdict verdict;
    uint32_t k, up;               // how the remaining levels are split between the tile and the cone (kSViewsLaunch only)
    char text[256];               // the refusal's message; empty on HGI_OK
};

// The rules of the launch entry in the header's order.  No HIP call, no allocation; `d_plan` is judged as an address only.
inline SViewsLaunchJudged sviews_judge(const void *d_plan, const hgi_sviews_info *info, uint32_t levels, hgi_interp interp)
{
    SViewsLaunchJudged j;
    j.status = HGI_OK;
    j.verdict = kSViewsEmpty;
    j.k = j.up = 0;
    j.text[0] = 0;
    // a plan of no grid succeeds and does nothing, whatever the other arguments
    if (info && info->magic == HGI_SVIEWS_MAGIC && info->count == 0 && sviews_info_consistent(*info)) return j;
    auto refuse = [&](hgi_status st, SViewsLaunchVerdict v) -> SViewsLaunchJudged & {
        j.status = st;
        j.verdict = v;
        return j;
    };
    // ---- HGI_EINVAL ----
    if (!info) {
        snprintf(j.text, sizeof(j.text), "info is NULL");
        return refuse(HGI_EINVAL, kSViewsInfoNull);
    }
    if (!sviews_info_consistent(*info)) {
        snprintf(j.text, sizeof(j.text), "info is not what hgi_sviews_plan wrote (magic, shift, sizes and offsets against the count %u, block count)", info->count);
        return refuse(HGI_EINVAL, kSViewsInfo);
    }
    if (!d_plan) {
        snprintf(j.text, sizeof(j.text), "d_plan is NULL");
        return refuse(HGI_EINVAL, kSViewsPlanNull);
    }
    if (reinterpret_cast<uintptr_t>(d_plan) % 16 != 0) {
        snprintf(j.text, sizeof(j.text), "d_plan is not 16-byte aligned");
        return refuse(HGI_EINVAL, kSViewsPlanAlign);
    }
    if (levels > 31) {
        snprintf(j.text, sizeof(j.text), "levels %u out of range 0..=31", levels);
        return refuse(HGI_EINVAL, kSViewsLevelsRange);
    }
    if (interp != HGI_INTERP_LEFTTOP && interp != HGI_INTERP_CROSSED) {
        snprintf(j.text, sizeof(j.text), "interpolator %d unknown (0 = LeftTop, 1 = Crossed)", (int)interp);
        return refuse(HGI_EINVAL, kSViewsInterp);
    }
    // ---- HGI_EUNSUPPORTED ----
    if (levels == 0) {
        snprintf(j.text, sizeof(j.text), "levels 0: nothing to decode (compose one scaled decode per view)");
        return refuse(HGI_EUNSUPPORTED, kSViewsLevelsZero);
    }
    if (levels <= info->shift) {
        snprintf(j.text, sizeof(j.text), "levels %u <= shift %u: the result is the grid's own lattice, a strided gather with no kernel here (compose one scaled decode per view)",
                 levels, info->shift);
        return refuse(HGI_EUNSUPPORTED, kSViewsGather);
    }
    if (levels - info->shift >= 9) {
        snprintf(j.text, sizeof(j.text), "levels %u - shift %u: one launch serves 1..=8 remaining levels (compose one scaled decode per view)", levels, info->shift);
        return refuse(HGI_EUNSUPPORTED, kSViewsDepth);
    }
    j.verdict = kSViewsLaunch;
    split_levels(levels - info->shift, &j.k, &j.up);
    return j;
}

}  // namespace hgi
