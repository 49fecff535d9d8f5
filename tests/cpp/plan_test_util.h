// What the stand-alone plan programs share (test_pitched_plan.cpp, test_{recon,map,typed,requant}_plan.cpp, test_sides.cpp):
// the random numbers, CHECK and the block-by-block walk of a pitched launch.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../rustyhgi_amd/csrc/hgi_pitched.h"

namespace {

uint64_t g_x = 0x9E3779B97F4A7C15ull;
uint64_t rnd()
{
    g_x ^= g_x << 13;
    g_x ^= g_x >> 7;
    g_x ^= g_x << 17;
    return g_x;
}
uint64_t rnd_in(uint64_t lo, uint64_t hi) { return lo + rnd() % (hi - lo + 1); }

int g_bad = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            if (g_bad < 20) {                              \
                std::printf("FAIL %s: ", #cond);           \
                std::printf(__VA_ARGS__);                  \
                std::printf("\n");                         \
            }                                              \
            ++g_bad;                                       \
        }                                                  \
    } while (0)

// One side of a launch as a kernel addresses it: the 32-bit pitch it multiplies with, the pitch it stands for, bytes per element.
struct WalkSide {
    const char *name;
    uint32_t pitch32;
    uint64_t pitch;
    uint32_t elem;
};

// Every block of a launch walked through pitched_tile(): every tile of every frame covered exactly once, interior tiles with
// their body inside the image (and only on a fast plan), on a fast plan no ragged tile with its body inside, idle blocks only
// in the padding behind the ragged tiles; on each of the `n` sides the tile's origin formed in 32-bit arithmetic, as the kernel
// forms it, equals the one formed in 64 bits.  per_tile(t, b): the caller's further checks on block b's tile.
template <class PerTile>
void walk_launch(int i, const hgi::PitchedPlan &p, uint32_t width, uint32_t height, uint32_t batch, const WalkSide *sides, int n, PerTile per_tile)
{
    const uint64_t tpf = (uint64_t)p.tx * p.ty, blocks = hgi::pitched_blocks(p);
    CHECK(blocks == ((p.nedge + 7u) & ~7u) + p.nf, "case %d: blocks", i);
    std::vector<uint8_t> seen((size_t)(tpf * batch), 0);
    uint64_t idle = 0;
    for (uint64_t b = 0; b < blocks; ++b) {
        const hgi::PitchedTile t = hgi::pitched_tile(p, (uint32_t)b);
        if (t.idle) {
            CHECK(b >= p.nedge && b < ((p.nedge + 7u) & ~7u), "case %d: idle block %llu outside the padding", i, (unsigned long long)b);
            ++idle;
            continue;
        }
        CHECK(t.frame < batch && t.X0 % 128 == 0 && t.Y0 % 64 == 0 && t.X0 < width && t.Y0 < height,
              "case %d: block %llu -> frame %u tile (%u, %u)", i, (unsigned long long)b, t.frame, t.X0, t.Y0);
        if (!(t.frame < batch && t.X0 < width && t.Y0 < height)) continue;
        const bool inside = (uint64_t)t.X0 + 128 <= width && (uint64_t)t.Y0 + 64 <= height;
        if (!t.edge) CHECK(inside && p.fast, "case %d: interior block %llu is ragged", i, (unsigned long long)b);
        if (t.edge && p.fast) CHECK(!inside, "case %d: ragged block %llu is interior", i, (unsigned long long)b);
        for (int s = 0; s < n; ++s) {
            const uint32_t base = t.Y0 * sides[s].pitch32 + t.X0 * sides[s].elem;
            CHECK(base == (uint64_t)t.Y0 * sides[s].pitch + (uint64_t)t.X0 * sides[s].elem, "case %d: %s side: tile origin wraps", i, sides[s].name);
        }
        per_tile(t, b);
        uint8_t &s = seen[(size_t)(t.frame * tpf + (uint64_t)(t.Y0 / 64) * p.tx + t.X0 / 128)];
        CHECK(s == 0, "case %d: tile covered twice", i);
        s = 1;
    }
    CHECK(idle == ((p.nedge + 7u) & ~7u) - p.nedge, "case %d: %llu idle blocks", i, (unsigned long long)idle);
    for (size_t k = 0; k < seen.size(); ++k) CHECK(seen[k] == 1, "case %d: tile %zu not covered", i, k);
}

inline void walk_launch(int i, const hgi::PitchedPlan &p, uint32_t width, uint32_t height, uint32_t batch, const WalkSide *sides, int n)
{
    walk_launch(i, p, width, height, batch, sides, n, [](const hgi::PitchedTile &, uint64_t) {});
}

// the bound of one side as include/hgi_*.h words it, restated
inline bool side_fits(uint32_t h, uint64_t pitch) { return pitch < (1ull << 32) && ((uint64_t)h + 192) * pitch + 1024 < (1ull << 32); }

}  // namespace
