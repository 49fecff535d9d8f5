// Frame lists (hgi_encode_u8_list_dev / hgi_decode_u8_list_dev): one launch over the 128 x 64 tiles of many frames of
// different shapes.  The host plan -- per frame exactly what fused_geom computes for a batch of one, and prefix sums of edge
// and interior tiles over the list -- and the block -> tile map the list kernels run (hgi_fused_list_dec.hip,
// hgi_fused_list_enc.hip).  Plain C++: tests/cpp/test_framelist_plan.cpp walks every block of a launch through the same
// functions with g++.
//
// Launch order: the edge tiles of all frames first, frame by frame, their count padded to a multiple of eight
// (b % 8 keeps labelling the XCD); then the interior tiles of all frames, frame-major and row-major, dealt to the eight XCDs
// in contiguous eighths (range_first).  A block finds its frame by a binary search over the prefix array of its kind:
// log2(count) dependent scalar loads, the same in every lane.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "hgi_fastdiv.h"

namespace hgi {

constexpr uint32_t kListTileW = 128, kListTileH = 64;   // the 64-row build of both directions

// One non-empty frame of a list launch (64 bytes: one scalar load of sixteen dwords).
struct ListFrame {
    uint64_t src, dst;            // the frame's input and output (device addresses)
    uint32_t width, height;
    uint32_t tiles_x, tiles_y;    // all tiles of the frame
    uint32_t full_x, full_y;      // tiles whose body lies inside the image (0 x 0: every tile takes the edge / checked path)
    uint32_t aligned;             // fused_geom's bits: 1 16-B rows and pointers, 2 check-free paths, 4 three extra read records
    uint32_t epf;                 // edge tiles: tiles_x * tiles_y - full_x * full_y
    FastDiv fd_fx;                // division by full_x (interior tiles, row-major)
};
static_assert(sizeof(ListFrame) == 64, "one 64-byte record per frame");

// What a list launch reads: the frame table and the two exclusive prefix arrays (edge and interior tiles of the frames in
// front of each), all in one device block; `count` non-empty frames.
struct ListArgs {
    const ListFrame *frames;
    const uint32_t *epre, *ipre;
    uint32_t count, nedge, nint;
};

// fused_geom for a batch of one (frame_stride = w * h, no row limit): src is the INPUT, whose last byte's page bounds the
// three-byte over-read of rows that are not a multiple of 4 bytes.  force_checked: the knobs build's HGI_FORCE_CHECKED.
inline ListFrame list_frame(uint64_t src, uint64_t dst, uint32_t w, uint32_t h, bool force_checked)
{
    ListFrame f;
    f.src = src;
    f.dst = dst;
    f.width = w;
    f.height = h;
    f.tiles_x = (uint32_t)(((uint64_t)w + kListTileW - 1) / kListTileW);
    f.tiles_y = (uint32_t)(((uint64_t)h + kListTileH - 1) / kListTileH);
    const uint64_t n = (uint64_t)w * h;
    const bool a16 = w % 16 == 0 && src % 16 == 0 && dst % 16 == 0;
    const bool fits32 = ((uint64_t)h + 2 * kListTileH + 64) * w + 1024 < (1ull << 32);
    const bool dword_rows = w % 4 == 0;
    const uint64_t end = src + n;
    const bool tail_ok = ((end - 1) >> 12) == ((end + 2) >> 12);
    const bool fast = n > 0 && fits32 && (dword_rows || tail_ok) && !force_checked;
    f.full_x = fast ? w / kListTileW : 0;
    f.full_y = fast ? h / kListTileH : 0;
    if (f.full_x == 0 || f.full_y == 0) f.full_x = f.full_y = 0;
    f.aligned = (a16 ? 1u : 0u) | (fast ? 2u : 0u) | (fast && !dword_rows ? 4u : 0u);
    f.epf = f.tiles_x * f.tiles_y - f.full_x * f.full_y;
    f.fd_fx = make_fastdiv(f.full_x ? f.full_x : 1u);
    return f;
}

// Tiles of a frame in 64 bits (the plan's limit check runs before anything is narrowed).
inline uint64_t list_tiles(uint32_t w, uint32_t h)
{
    return (((uint64_t)w + kListTileW - 1) / kListTileW) * (((uint64_t)h + kListTileH - 1) / kListTileH);
}

// Blocks of a launch: the edge tiles padded to a multiple of eight, then the interior tiles.
HGI_HD inline uint64_t list_blocks(uint64_t nedge, uint64_t nint) { return ((nedge + 7u) & ~(uint64_t)7u) + nint; }

// The plan of `n` frames (zero-size frames skipped): table, prefix arrays, totals.  `frames`, `epre`, `ipre` hold room for
// every non-empty frame.  Returns the number of non-empty frames.  The caller has checked that the list's tiles fit a launch
// (list_blocks(all tiles) < 2^31), so no 32-bit sum below can wrap.
inline uint32_t plan_list(const uint64_t *src, const uint64_t *dst, const uint32_t *w, const uint32_t *h, size_t n, bool force_checked,
                          ListFrame *frames, uint32_t *epre, uint32_t *ipre, uint32_t *nedge, uint32_t *nint)
{
    uint32_t m = 0, ne = 0, ni = 0;
    for (size_t i = 0; i < n; ++i) {
        if (w[i] == 0 || h[i] == 0) continue;
        const ListFrame f = list_frame(src[i], dst[i], w[i], h[i], force_checked);
        frames[m] = f;
        epre[m] = ne;
        ipre[m] = ni;
        ne += f.epf;
        ni += f.full_x * f.full_y;
        ++m;
    }
    *nedge = ne;
    *nint = ni;
    return m;
}

// The frame that holds tile t of a prefix array: the last i < count with pre[i] <= t (pre[0] == 0; frames without tiles of this
// kind repeat their successor's entry and are passed over).  Clamped to count - 1 whatever the table holds.  (`pre` is a
// pointer type: the kernels pass one into the constant address space, so that every probe is a scalar load.)
template <class P>
HGI_HD inline uint32_t list_find(P pre, uint32_t count, uint32_t t)
{
    uint32_t lo = 0, n = count;
    while (n > 1) {
        const uint32_t half = n >> 1;
        if (pre[lo + half] <= t) {
            lo += half;
            n -= half;
        } else {
            n = half;
        }
    }
    return count && lo >= count ? count - 1 : lo;
}

// XCD x's first position in a list of n tiles dealt in contiguous eighths (hgi_fused_impl.h range_first)
HGI_HD inline uint32_t list_range_first(uint32_t n, uint32_t x) { return x * (n >> 3) + (x < (n & 7u) ? x : (n & 7u)); }

struct ListBlock {
    bool edge, idle;
    uint32_t t;          // index in the edge list or the interior list
    uint32_t frame;      // index in the table
    uint32_t tx, ty;     // tile column and row in the frame
};

// Block b's kind and position in its list; nothing is loaded.
HGI_HD inline ListBlock list_role(uint32_t b, uint32_t nedge, uint32_t nint)
{
    ListBlock r;
    const uint32_t ne8 = (nedge + 7u) & ~7u;
    r.edge = b < ne8;
    r.idle = r.edge ? b >= nedge : b - ne8 >= nint;
    const uint32_t fb = b - ne8;
    r.t = r.edge ? (r.idle ? 0u : b) : list_range_first(nint, fb & 7u) + (fb >> 3);
    r.frame = r.tx = r.ty = 0;
    return r;
}

// The tile of a non-idle block inside frame F: edge tiles as edge_tile orders them (the columns right of the interior ones,
// every row; then the interior columns of the rows below), interior tiles row-major.
HGI_HD inline void list_tile(ListBlock &r, const ListFrame &F, uint32_t first)
{
    uint32_t i = r.t - first;
    if (r.edge) {
        const uint32_t wr = F.tiles_x - F.full_x, right = wr * F.tiles_y;
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

// The whole map, as the host test walks it (the kernels run list_role / list_find / list_tile with their loads placed early).
inline ListBlock list_block(uint32_t b, const ListArgs &a)
{
    ListBlock r = list_role(b, a.nedge, a.nint);
    if (r.idle || a.count == 0) return r;
    const uint32_t *pre = r.edge ? a.epre : a.ipre;
    r.frame = list_find(pre, a.count, r.t);
    list_tile(r, a.frames[r.frame], pre[r.frame]);
    return r;
}

// Overlap rule of the list calls on byte spans [p, p + n): outputs pairwise disjoint, no output meeting an input; inputs may
// overlap each other.  Sorted sweep, O(n log n).  Returns 0 (fine), 1 (two outputs meet) or 2 (an output meets an input);
// *a / *b: the list indices of a pair that does (the output first when one is).  Zero-size spans are ignored.
struct ListSpan {
    uint64_t lo, hi;
    size_t index;
    bool out;
};

inline int list_overlap(std::vector<ListSpan> &spans, size_t *a, size_t *b)
{
    std::sort(spans.begin(), spans.end(), [](const ListSpan &x, const ListSpan &y) { return x.lo < y.lo; });
    // every span meets each earlier one that reaches past its start: the furthest reach of the earlier outputs, and of all
    // earlier spans, decides (a span that reaches past s.lo without being an output is an input)
    uint64_t hi_any = 0, hi_out = 0;
    size_t at_any = 0, at_out = 0;
    for (const ListSpan &s : spans) {
        if (s.hi <= s.lo) continue;
        if (s.lo < hi_out) {
            *a = at_out;
            *b = s.index;
            return s.out ? 1 : 2;
        }
        if (s.out && s.lo < hi_any) {
            *a = s.index;
            *b = at_any;
            return 2;
        }
        if (s.hi > hi_any) hi_any = s.hi, at_any = s.index;
        if (s.out && s.hi > hi_out) hi_out = s.hi, at_out = s.index;
    }
    return 0;
}

}  // namespace hgi
