// Recon view lists (hgi_rviews_plan / hgi_rviews_encode_dev, include/hgi_rviews.h): the host plan of one launch over the
// 128 x 64 tiles of many frames that each bring a shape and THREE pitches of their own -- the image read, the grid and the
// reconstruction written -- and the launch's whole judgement.  It is the view lists' plan (../views/hgi_views_plan.h) with the
// third side of encode with reconstruction (../recon/hgi_recon_plan.h) per frame:
//   * the blob starts with the three arrays views_plan writes for the (src, grid) pairs, byte for byte -- the 64-byte ViewFrame
//     records, the edge prefix, the interior prefix -- so the launch order, the block -> tile map and the frame search are the
//     view lists' unchanged (view_block; list_role / list_find / view_tile and views_tile_launch on the device side);
//   * the ViewFrame record is full, so the third side stands in a parallel array behind them, at recon_offset =
//     views_blob_bytes(count): one 16-byte RViewSide per frame, the reconstruction's address and what extra_side / side_span
//     (../companion/hgi_sides.h) give for a batch of one -- the pitch and the num_records of its write descriptor;
//   * the aliasing test is that plan's sweep (views_aliasing) on three rectangles per entry; ViewRect::index carries the side.
// The bound of a side and the page rule are companion/hgi_sides.h's.  Plain C++, no HIP: tests/cpp/test_rviews_plan.cpp runs it
// with g++.
//
// This library has no byte-checked path: a list with an entry that does not take the 32-bit buffer path is refused
// (HGI_EUNSUPPORTED) and the caller composes one hgi_recon_encode_u8_dev call per view.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/hgi_rviews.h"
#include "../views/hgi_views_plan.h"

namespace hgi {

// The third side of one non-empty frame (16 bytes: one scalar 16-byte load).
struct RViewSide {
    uint64_t recon;               // the frame's reconstruction (device address)
    uint32_t pitch32, rec;        // write pitch (a one-row frame's: its width); num_records (span) of the write descriptor
};
static_assert(sizeof(RViewSide) == 16, "one 16-byte record per frame");

// What a launch reads (kernel argument, by value): the view lists' three arrays and the parallel array of third sides.
struct RViewArgs {
    ViewArgs v;
    const RViewSide *recon;
};

// ---- the frame search ---------------------------------------------------------------------------------------------------------
// list_find's result (../csrc/hgi_framelist.h: the last i < count with pre[i] <= t of a prefix array, pre[0] == 0, entries that
// repeat passed over; below count whatever the table holds) as a descent over fixed steps, 2^30 down to 1, with no loop left in
// the caller once it is unrolled: a step is a uniform compare and, where lo + step is an entry of the array, one probe --
// about log2(count) probes, as list_find makes.  The kernels of this library search with it because a cycle in
// front of k_enc_recon's body, of whatever content, costs the cone kernels three VGPRs (Registers); the host
// walk (view_block) and every other library search with list_find, and tests/cpp/test_rviews_plan.cpp holds the two equal.
// count < 2^31 (the block count of a launch): lo + step does not wrap.
template <class P>
HGI_HD inline uint32_t rview_find(P pre, uint32_t count, uint32_t t)
{
    uint32_t lo = 0;
#if defined(__clang__)
#pragma unroll
#endif
    for (uint32_t step = 1u << 30; step; step >>= 1)
        if (lo + step < count && pre[lo + step] <= t) lo += step;
    return lo;
}

// ---- the blob ---------------------------------------------------------------------------------------------------------------
inline uint64_t rviews_recon_offset(uint64_t count) { return views_blob_bytes(count); }
inline uint64_t rviews_blob_bytes(uint64_t count) { return views_blob_bytes(count) + 16 * count; }

inline hgi_view_pair rview_pair(const hgi_rview_triple &t)
{
    const hgi_view_pair v = {t.src, t.grid, t.width, t.height, t.src_pitch, t.grid_pitch};
    return v;
}

// `t`: a non-empty entry that passed every rule (all three sides fit 32 bits).
inline RViewSide rview_side(const hgi_rview_triple &t)
{
    const uint64_t rp = t.height > 1 ? t.recon_pitch : t.width;
    const ExtraSide x = extra_side(true, rp, side_span(t.width, t.height, rp), 0);
    const RViewSide s = {t.recon, x.pitch32, x.rec};
    return s;
}

// The arrays of a blob that lies at `base` (host: the caller's memory; launch: the device address), per `info`.
inline RViewArgs rview_args(const void *base, const hgi_rviews_info &info)
{
    const uint8_t *b = static_cast<const uint8_t *>(base);
    RViewArgs a;
    a.v.frames = reinterpret_cast<const ViewFrame *>(b + info.records_offset);
    a.v.epre = reinterpret_cast<const uint32_t *>(b + info.edge_prefix_offset);
    a.v.ipre = reinterpret_cast<const uint32_t *>(b + info.interior_prefix_offset);
    a.v.count = info.count;
    a.v.nedge = info.edge_tiles;
    a.v.nint = info.interior_tiles;
    a.recon = reinterpret_cast<const RViewSide *>(b + info.recon_offset);
    return a;
}

// What a launch checks of the host struct it is handed: the magic, the sizes and offsets against the count, the block count.
inline bool rviews_info_consistent(const hgi_rviews_info &i)
{
    if (i.magic != HGI_RVIEWS_MAGIC || i.reserved != 0) return false;
    if (i.plan_bytes != rviews_blob_bytes(i.count) || i.records_offset != views_records_offset() ||
        i.edge_prefix_offset != views_epre_offset(i.count) || i.interior_prefix_offset != views_ipre_offset(i.count) ||
        i.recon_offset != rviews_recon_offset(i.count))
        return false;
    if (i.count == 0) return i.edge_tiles == 0 && i.interior_tiles == 0 && i.max_width == 0;
    const uint64_t tiles = (uint64_t)i.edge_tiles + i.interior_tiles;
    return i.max_width != 0 && tiles >= i.count && list_blocks(i.edge_tiles, i.interior_tiles) + 8 < (1ull << 31);
}

enum RViewsVerdict {
    kRViewsOk = 0,
    // HGI_EINVAL
    kRViewsNullEntry, kRViewsSrcPitch, kRViewsGridPitch, kRViewsReconPitch, kRViewsTiles, kRViewsOutOut, kRViewsOutIn,
    // HGI_EUNSUPPORTED
    kRViewsFits32, kRViewsTail,
};

enum RViewsSide { kRViewsGrid = 0, kRViewsRecon = 1 };

struct RViewsJudged {
    RViewsVerdict verdict;
    size_t a, b;                  // the list index the verdict names; for an aliasing pair the output first, then the other view
    int side_a, side_b;           // an aliasing pair: which output `a` is; which output `b` is (kRViewsOutOut only)
    bool mixed_pitch;             // an aliasing pair that was refused without being judged: spans meet, pitches differ
};

// ---- the plan ----------------------------------------------------------------------------------------------------------------
// Every rule of a list in the order of include/hgi_rviews.h.  triples != nullptr or n == 0; the entry point has judged the NULL
// arguments and plan_bytes >= rviews_blob_bytes(n).  On kRViewsOk the blob is written to h_plan and *info filled; otherwise
// neither is touched.  Nothing is allocated before the tile count is known to fit.
inline RViewsJudged rviews_plan(const hgi_rview_triple *triples, size_t n, void *h_plan, hgi_rviews_info *info)
{
    RViewsJudged j = {kRViewsOk, 0, 0, 0, 0, false};
    auto refuse = [&](RViewsVerdict v, size_t a) {
        j.verdict = v;
        j.a = j.b = a;
        return j;
    };
    uint64_t tiles = 0, count = 0;
    bool too_many = false;
    for (size_t i = 0; i < n; ++i) {
        const hgi_rview_triple &t = triples[i];
        if (t.width == 0 || t.height == 0) continue;
        if (!t.src || !t.grid || !t.recon) return refuse(kRViewsNullEntry, i);
        if (t.height > 1 && t.src_pitch < t.width) return refuse(kRViewsSrcPitch, i);
        if (t.height > 1 && t.grid_pitch < t.width) return refuse(kRViewsGridPitch, i);
        if (t.height > 1 && t.recon_pitch < t.width) return refuse(kRViewsReconPitch, i);
        ++count;
        // once per entry: one tile writes both outputs
        if (!too_many) tiles += list_tiles(t.width, t.height);      // (a frame has fewer than 2^52 tiles: no wrap below 2^31 frames' worth)
        too_many = too_many || list_blocks(tiles, 0) + 8 >= (1ull << 31);
    }
    if (too_many) return refuse(kRViewsTiles, 0);
    if (count) {
        // three rectangles per entry; the index of a rectangle is 2 * (list index) + (1 for the reconstruction)
        std::vector<ViewRect> rects;
        rects.reserve(3 * (size_t)count);
        for (size_t i = 0; i < n; ++i) {
            const hgi_rview_triple &t = triples[i];
            if (t.width == 0 || t.height == 0) continue;
            rects.push_back(view_rect(t.src, t.width, t.height, t.src_pitch, 2 * i, false));
            rects.push_back(view_rect(t.grid, t.width, t.height, t.grid_pitch, 2 * i + kRViewsGrid, true));
            rects.push_back(view_rect(t.recon, t.width, t.height, t.recon_pitch, 2 * i + kRViewsRecon, true));
        }
        const ViewsJudged a = views_aliasing(rects);
        if (a.verdict != kViewsOk) {
            j.verdict = a.verdict == kViewsOutOut ? kRViewsOutOut : kRViewsOutIn;
            j.a = a.a / 2;
            j.b = a.b / 2;
            j.side_a = (int)(a.a & 1);
            j.side_b = (int)(a.b & 1);
            j.mixed_pitch = a.mixed_pitch;
            return j;
        }
    }
    for (size_t i = 0; i < n; ++i) {
        const hgi_rview_triple &t = triples[i];
        if (t.width == 0 || t.height == 0) continue;
        const uint64_t sp = t.height > 1 ? t.src_pitch : t.width, gp = t.height > 1 ? t.grid_pitch : t.width,
                       rp = t.height > 1 ? t.recon_pitch : t.width;
        const uint64_t P = sp > gp ? (sp > rp ? sp : rp) : (gp > rp ? gp : rp);
        if (!side_fits32(t.height, P)) return refuse(kRViewsFits32, i);
        if (t.width % 4 != 0 && !tail_in_page(t.src, t.width, t.height, t.src_pitch, 0, 1, 3)) return refuse(kRViewsTail, i);
    }
    // every rule holds: the blob
    hgi_rviews_info o;
    memset(&o, 0, sizeof(o));
    o.magic = HGI_RVIEWS_MAGIC;
    o.count = (uint32_t)count;
    o.plan_bytes = rviews_blob_bytes(count);
    o.records_offset = views_records_offset();
    o.edge_prefix_offset = views_epre_offset(count);
    o.interior_prefix_offset = views_ipre_offset(count);
    o.recon_offset = rviews_recon_offset(count);
    if (count) {
        uint8_t *blob = static_cast<uint8_t *>(h_plan);
        memset(blob, 0, (size_t)o.plan_bytes);
        uint32_t m = 0, ne = 0, ni = 0, wmax = 0;
        for (size_t i = 0; i < n; ++i) {
            const hgi_rview_triple &t = triples[i];
            if (t.width == 0 || t.height == 0) continue;
            const hgi_view_pair v = rview_pair(t);
            const PitchedPlan p = view_pitched_plan(v);
            const ViewFrame f = view_frame(v, p);
            const RViewSide s = rview_side(t);
            memcpy(blob + o.records_offset + 64 * (uint64_t)m, &f, 64);
            memcpy(blob + o.edge_prefix_offset + 4 * (uint64_t)m, &ne, 4);
            memcpy(blob + o.interior_prefix_offset + 4 * (uint64_t)m, &ni, 4);
            memcpy(blob + o.recon_offset + 16 * (uint64_t)m, &s, 16);
            ne += p.epf;
            ni += p.ipf;
            wmax = t.width > wmax ? t.width : wmax;
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
enum RViewsLaunchVerdict {
    kRViewsLaunch = 0,            // every rule holds: k / up / ident are set
    kRViewsEmpty,                 // a plan of no frame: HGI_OK, nothing launched
    // HGI_EINVAL
    kRViewsInfoNull, kRViewsInfo, kRViewsPlanNull, kRViewsPlanAlign, kRViewsLutNull, kRViewsLevelsRange, kRViewsInterp,
    // HGI_EUNSUPPORTED
    kRViewsLevels,
};

struct RViewsLaunchJudged {
    hgi_status status;
    RViewsLaunchVerdict verdict;
    uint32_t k, up;               // how the pyramid is split between the tile and the cone (kRViewsLaunch only)
    bool ident;                   // the identity table: the residual-only instantiation (kRViewsLaunch only)
    char text[256];               // the refusal's message; empty on HGI_OK
};

// The rules of the launch entry in the header's order.  No HIP call, no allocation; `d_plan` is judged as an address only and
// `lut` is read (256 bytes of host memory) only behind every rule.
inline RViewsLaunchJudged rviews_judge(const void *d_plan, const hgi_rviews_info *info, uint32_t levels, hgi_interp interp, const uint8_t *lut)
{
    RViewsLaunchJudged j;
    j.status = HGI_OK;
    j.verdict = kRViewsEmpty;
    j.k = j.up = 0;
    j.ident = false;
    j.text[0] = 0;
    // a plan of no frame succeeds and does nothing, whatever the other arguments
    if (info && info->magic == HGI_RVIEWS_MAGIC && info->count == 0 && rviews_info_consistent(*info)) return j;
    auto refuse = [&](hgi_status st, RViewsLaunchVerdict v) -> RViewsLaunchJudged & {
        j.status = st;
        j.verdict = v;
        return j;
    };
    // ---- HGI_EINVAL ----
    if (!info) {
        snprintf(j.text, sizeof(j.text), "info is NULL");
        return refuse(HGI_EINVAL, kRViewsInfoNull);
    }
    if (!rviews_info_consistent(*info)) {
        snprintf(j.text, sizeof(j.text), "info is not what hgi_rviews_plan wrote (magic, sizes and offsets against the count %u, block count)", info->count);
        return refuse(HGI_EINVAL, kRViewsInfo);
    }
    if (!d_plan) {
        snprintf(j.text, sizeof(j.text), "d_plan is NULL");
        return refuse(HGI_EINVAL, kRViewsPlanNull);
    }
    if (reinterpret_cast<uintptr_t>(d_plan) % 16 != 0) {
        snprintf(j.text, sizeof(j.text), "d_plan is not 16-byte aligned");
        return refuse(HGI_EINVAL, kRViewsPlanAlign);
    }
    if (!lut) {
        snprintf(j.text, sizeof(j.text), "lut is NULL");
        return refuse(HGI_EINVAL, kRViewsLutNull);
    }
    if (levels > 31) {
        snprintf(j.text, sizeof(j.text), "levels %u out of range 0..=31", levels);
        return refuse(HGI_EINVAL, kRViewsLevelsRange);
    }
    if (interp != HGI_INTERP_LEFTTOP && interp != HGI_INTERP_CROSSED) {
        snprintf(j.text, sizeof(j.text), "interpolator %d unknown (0 = LeftTop, 1 = Crossed)", (int)interp);
        return refuse(HGI_EINVAL, kRViewsInterp);
    }
    // ---- HGI_EUNSUPPORTED ----
    if (levels == 0 || levels > 8) {
        snprintf(j.text, sizeof(j.text), "levels %u: one launch serves 1..=8 levels (compose one encode with reconstruction per view)", levels);
        return refuse(HGI_EUNSUPPORTED, kRViewsLevels);
    }
    j.verdict = kRViewsLaunch;
    split_levels(levels, &j.k, &j.up);
    j.ident = true;
    for (int i = 0; i < 256; ++i) j.ident = j.ident && lut[i] == i;
    return j;
}

// What the launcher makes of a judged info: one block per tile of the list, the ragged tiles padded to a multiple of eight.
inline uint64_t rviews_blocks(const hgi_rviews_info &info) { return list_blocks(info.edge_tiles, info.interior_tiles); }

}  // namespace hgi
