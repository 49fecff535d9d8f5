// The codec level by level, restated for the reference launches (sim_kernels.cpp): seed, one encode level, one decode level,
// out-of-image corners read 0, table plus overflow fallback.  Written from the codec's definition, not from the kernels;
// test_host_routes.cpp first asserts whole frames coded with these functions equal to oracle/hgi_oracle.c.
//
// Level `s` (its log2 sub-step; the frame's levels run s = levels - 1 ... 0) visits every point whose coordinates are both
// multiples of 2^s and not both multiples of 2^(s + 1); its prediction reads the four points of the enclosing 2^(s + 1) cell's
// corners, all of which coarser levels (or the seed) have finished.  So the order inside a level does not matter.
#pragma once
#include <stdint.h>
#include <string.h>

namespace ref {

inline uint8_t at(const uint8_t *img, uint32_t w, uint32_t h, uint64_t x, uint64_t y) { return x < w && y < h ? img[y * w + x] : 0; }

inline uint8_t predict(int interp, const uint8_t *img, uint32_t w, uint32_t h, uint64_t x, uint64_t y, uint32_t s)
{
    const uint64_t step = (uint64_t)2 << s, x0 = x & ~(step - 1), y0 = y & ~(step - 1);
    if (interp == 0) return img[y0 * w + x0];   // LeftTop: the cell's own corner, always inside
    const unsigned a = at(img, w, h, x0, y0), b = at(img, w, h, x0, y0 + step), c = at(img, w, h, x0 + step, y0),
                   d = at(img, w, h, x0 + step, y0 + step);
    // the four rounded-up means of neighbouring corners, then their truncated mean
    return (uint8_t)((((a + c + 1) >> 1) + ((d + b + 1) >> 1) + ((b + a + 1) >> 1) + ((d + c + 1) >> 1)) >> 2);
}

template <class F>
inline void for_level(uint32_t w, uint32_t h, uint32_t s, F f)
{
    const uint64_t sub = (uint64_t)1 << s, step = sub << 1;
    for (uint64_t y = 0; y < h; y += sub) {
        const bool on = (y & (step - 1)) == 0;
        for (uint64_t x = on ? sub : 0; x < w; x += on ? step : sub) f(x, y);
    }
}

// the stride-2^levels lattice is carried as it is
inline void seed(const uint8_t *src, uint8_t *dst, uint32_t w, uint32_t h, uint32_t levels)
{
    const uint64_t step = (uint64_t)1 << levels;
    for (uint64_t y = 0; y < h; y += step)
        for (uint64_t x = 0; x < w; x += step) dst[y * w + x] = src[y * w + x];
}

inline void decode_level(const uint8_t *grid, uint8_t *img, uint32_t w, uint32_t h, uint32_t s, int interp)
{
    for_level(w, h, s, [&](uint64_t x, uint64_t y) { img[y * w + x] = (uint8_t)(predict(interp, img, w, h, x, y, s) + grid[y * w + x]); });
}

// rec: the image on entry at the points of this and finer levels, the reconstruction at coarser ones; this level's points
// become reconstruction.
inline void encode_level(uint8_t *rec, uint8_t *grid, uint32_t w, uint32_t h, uint32_t s, int interp, const uint8_t lut[256])
{
    for_level(w, h, s, [&](uint64_t x, uint64_t y) {
        const unsigned p = predict(interp, rec, w, h, x, y, s);
        const uint8_t diff = (uint8_t)(rec[y * w + x] - p);
        uint8_t q = lut[diff];
        if ((p + q > 255) != (p + diff > 255)) q = diff;   // the table would flip the wrap-around: keep the exact residual
        grid[y * w + x] = q;
        rec[y * w + x] = (uint8_t)(p + q);
    });
}

inline void decode(const uint8_t *grid, uint8_t *img, uint32_t w, uint32_t h, uint32_t levels, int interp)
{
    seed(grid, img, w, h, levels);
    for (uint32_t s = levels; s-- > 0;) decode_level(grid, img, w, h, s, interp);
}

// rec: w * h bytes of scratch; holds the reconstruction afterwards
inline void encode(const uint8_t *img, uint8_t *grid, uint8_t *rec, uint32_t w, uint32_t h, uint32_t levels, int interp, const uint8_t lut[256])
{
    memcpy(rec, img, (size_t)w * h);
    seed(img, grid, w, h, levels);
    for (uint32_t s = levels; s-- > 0;) encode_level(rec, grid, w, h, s, interp, lut);
}

}  // namespace ref
