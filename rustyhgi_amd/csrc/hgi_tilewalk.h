// The block -> tile walk of the uniform tile kernels (hgi_fused_impl.h: k_dec_tiles / k_enc_tiles): the launch's tile lists,
// what the host derives from them once per launch (finish_grid) and the index arithmetic every block runs on them
// (walk_block_role, walk_fast_tile, walk_edge_tile).  Plain C++: tests/cpp/test_tilewalk.cpp runs it with g++.  The kernels
// pass blockIdx.x in and keep what only a device can do (readfirstlane, the early scalar loads) next to their calls.
//
// Launch order: the ragged tiles of all frames first (a frame's right columns, then its bottom rows; their count padded to a
// multiple of eight so that b % 8 keeps labelling the XCD), then the interior tiles in band order -- bands of `band` tile
// rows, column-major inside a band, the last band of a frame taking the rows that are left -- dealt to the eight XCDs either
// in contiguous eighths (xmode 0) or as whole bands round-robin with a contiguously split tail (xmode 1).
#pragma once
#include <stdint.h>

#include "hgi_fastdiv.h"

#if defined(__HIPCC__)
#define HGI_WALK_FN __host__ __device__ __forceinline__
#else
#define HGI_WALK_FN inline
#endif
#ifndef HGI_TILE_ORDER
#define HGI_TILE_ORDER 0      // order of the interior tiles inside a frame: 0 row-major (experiment), 3 column-major bands (shipped; set by the direction's unit)
#endif

namespace hgi {
namespace {

// Tile lists.  `full_x` x `full_y` tiles per frame lie entirely inside the image: the fast kernels walk
// those; the checked path takes the rest (right column first, then the bottom rows).
// (FastDiv / make_fastdiv / fdiv: hgi_fastdiv.h -- the block -> tile index math divides by launch-wide constants only)
struct TileGrid {
    uint32_t tiles_x, tiles_y;   // all tiles of a frame
    uint32_t full_x, full_y;     // tiles whose body is inside the image (0 x 0 when the fast path is off)
    uint32_t nfast, nedge;       // totals over the batch
    uint32_t reverse;            // walk the interior tile list backwards (speed only: see launch_decode_fused)
    uint32_t band;               // tile rows per band of the column-major walk (walk_fast_tile)
    uint32_t xmode;              // how the band-ordered tile list is dealt to the XCDs (walk_block_role)
    // derived by finish_grid() on the host, so that the kernels neither divide nor re-derive launch constants:
    uint32_t ex, nf;             // interior tile columns / interior tiles the walk runs on
    uint32_t tpf, P, nfull, rem_rows;   // tiles per frame; per band; in a frame's whole bands; rows of its last, shorter band
    uint32_t rr_own, rr_tail0;   // round-robin dealing: blocks per XCD that belong to whole rounds of eight bands; first tile behind them
    FastDiv fd_tpf, fd_P, fd_band, fd_rem, fd_ex;
#ifdef HGI_TIMELINE
    uint64_t *timeline;          // experiment builds (tools/timeline.py): eight u64 per block -- start, staged, end, hardware id, entry
#endif
};

struct WalkTile {
    uint32_t frame, tx, ty;      // tile column and row inside the frame
};

// XCD-aware block -> tile map.  Workgroups are dealt round-robin over the 8 XCDs (b % 8 labels the XCD a
// block runs on), so XCD x gets the x-th contiguous eighth of the row-major tile list: x-neighbours
// (which share halo lines) and consecutive tile rows land in the same XCD's L2.  Speed only, never
// correctness.
HGI_WALK_FN uint32_t range_first(uint32_t ntiles, uint32_t x) { return x * (ntiles >> 3) + (x < (ntiles & 7u) ? x : (ntiles & 7u)); }

// Position `t` of the walk -> position in the band-ordered list of interior tiles
HGI_WALK_FN uint32_t walk_position(uint32_t t, const TileGrid &g) { return g.reverse ? g.nf - 1u - t : t; }

// Position t of the band-ordered list of interior tiles -> its tile
HGI_WALK_FN WalkTile walk_fast_tile(uint32_t t, const TileGrid &g)
{
    WalkTile tl;
    tl.frame = fdiv(t, g.fd_tpf);
    const uint32_t tt = t - tl.frame * g.tpf;
    uint32_t ty, tx;
#if HGI_TILE_ORDER == 0          // row-major (experiment)
    ty = fdiv(tt, g.fd_ex);
    tx = tt - ty * g.ex;
#else
    // Bands of g.band tile rows, column-major inside a band: x-neighbours are dispatched `rows` tiles apart,
    // y-neighbours next to each other.  The last band of a frame takes the rows that are left.
    {
        uint32_t rows, row0, r;
        if (tt < g.nfull) {
            const uint32_t band = fdiv(tt, g.fd_P);
            r = tt - band * g.P;
            row0 = band * g.band;
            rows = g.band;
            tx = fdiv(r, g.fd_band);
        } else {
            rows = g.rem_rows;
            r = tt - g.nfull;
            row0 = g.full_y - rows;
            tx = fdiv(r, g.fd_rem);
        }
        ty = row0 + (r - tx * rows);
    }
#endif
    tl.tx = tx;
    tl.ty = ty;
    return tl;
}

HGI_WALK_FN WalkTile walk_edge_tile(uint32_t e, const TileGrid &g)
{
    const uint32_t right = (g.tiles_x - g.full_x) * g.tiles_y;          // tiles with tx >= full_x
    const uint32_t epf = right + g.full_x * (g.tiles_y - g.full_y);     // + tiles with ty >= full_y, tx < full_x
    WalkTile tl;
    tl.frame = e / epf;
    uint32_t i = e - tl.frame * epf, tx, ty;
    if (i < right) {
        const uint32_t w = g.tiles_x - g.full_x;
        ty = i / w;
        tx = g.full_x + (i - ty * w);
    } else {
        i -= right;
        ty = g.full_y + i / g.full_x;
        tx = i % g.full_x;
    }
    tl.tx = tx;
    tl.ty = ty;
    return tl;
}

// One block (= one wave) per tile, ONE launch per batch.  The first blocks take the ragged tiles
// (their count padded to a multiple of 8 so that b % 8 keeps labelling the XCD), so the slow tiles
// start first and overlap the interior ones; the interior tiles follow in XCD-contiguous order.
// (A persistent variant -- resident waves pulling tiles from per-XCD atomic counters and prefetching
// the next tile into registers -- was built and measured: not faster on MI355X, see DESIGN.md
// "Scheduling".)
struct BlockRole {
    bool edge, idle;
    uint32_t index;       // edge tile index, or position of the interior tile in the XCD-contiguous order
};

// b: the block's index in the launch
HGI_WALK_FN BlockRole walk_block_role(uint32_t b, const TileGrid &g)
{
    const uint32_t ne8 = (g.nedge + 7u) & ~7u;
    BlockRole r;
    r.edge = b < ne8;
    r.idle = r.edge && b >= g.nedge;
    const uint32_t fb = b - ne8;
    r.index = r.edge ? b : range_first(g.nf, fb & 7u) + (fb >> 3);
    // Which tiles the eight XCDs work on at one time (speed only; g.xmode, host policy xcd_mode()).  0: each XCD walks its
    // own contiguous eighth of the band-ordered list -- eight places an eighth of the batch apart, a power-of-two distance
    // on power-of-two frames.  1: whole bands dealt round-robin, so the XCDs work on eight CONSECUTIVE bands (16384^2:
    // -10 % encode, -9 % decode; 64 x 4096^2: -1.5 ... -1.8 %; profiles/r03_ab_xcd.txt); what is left after the last
    // multiple of eight bands is split contiguously as in mode 0.  (finish_grid() clears xmode when a frame's rows do not
    // divide into whole bands.)
    if (!r.edge && g.xmode == 1) {
        const uint32_t x = fb & 7u, sq = fb >> 3;
        if (sq < g.rr_own) {
            const uint32_t round = fdiv(sq, g.fd_P);
            r.index = (round * 8u + x) * g.P + (sq - round * g.P);
        } else {
            r.index = g.rr_tail0 + range_first(g.nf - g.rr_tail0, x) + (sq - g.rr_own);
        }
    }
    return r;
}

// Everything the kernels would otherwise derive per block from the launch's constants (and the divisions by them).
inline void finish_grid(TileGrid &g)
{
    g.ex = g.full_x;
    g.nf = g.nfast;
    if (g.band < 1) g.band = 1;
    g.tpf = g.ex * g.full_y;
    g.P = g.band * g.ex;
    g.nfull = (g.full_y / g.band) * g.P;
    g.rem_rows = g.full_y % g.band;
    g.fd_tpf = make_fastdiv(g.tpf);
    g.fd_P = make_fastdiv(g.P);
    g.fd_band = make_fastdiv(g.band);
    g.fd_rem = make_fastdiv(g.rem_rows);
    g.fd_ex = make_fastdiv(g.ex);
    g.rr_own = g.rr_tail0 = 0;
    if (g.xmode != 1 || g.rem_rows != 0 || g.P == 0 || g.nf == 0) {
        g.xmode = 0;
    } else {
        const uint32_t nb8 = (g.nf / g.P) & ~7u;          // bands in whole rounds of eight
        g.rr_own = (nb8 >> 3) * g.P;
        g.rr_tail0 = nb8 * g.P;
    }
}

}  // namespace
}  // namespace hgi
