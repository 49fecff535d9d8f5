// How many tiles of a decode a CU holds at one time: the numbers, the rule and the LDS padding that enforces it, once, for
// every decode launcher of the core and of the companion libraries.  Plain C++, no HIP header: the host test
// (tests/cpp/test_launch_policy.cpp) compiles it with g++.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "hgi_knobs.h"

#ifndef HGI_DEC_SHALLOW_WAVES
#define HGI_DEC_SHALLOW_WAVES 20  // resident tiles per CU asked for on decodes 1-8 rounds deep (dec_resident_tiles)
#endif
#ifndef HGI_DEC_DEEP_WAVES
#define HGI_DEC_DEEP_WAVES 16     // ... and on deeper ones (launches that rebuild levels in the kernel or start from seed planes)
#endif
#ifndef HGI_DEC_STREAM_WAVES
#define HGI_DEC_STREAM_WAVES 10   // resident tiles per CU of a plain decode (the tile holds the pyramid) of 8 192 tiles and more, rows up
#endif                            // to 4 096 pixels and up to four levels ...
#ifndef HGI_DEC_STREAM_WAVES_WIDE
#define HGI_DEC_STREAM_WAVES_WIDE 12   // ... and on wider rows or five levels
#endif
#ifndef HGI_DEC_STREAM_WAVES_L1
#define HGI_DEC_STREAM_WAVES_L1 8      // ... and at ONE level (the finest pass alone: a tile's lifetime is shortest there)
#endif

namespace hgi {

// Dynamic LDS of a launch padded so that at most `waves` blocks fit a CU (160 KiB of LDS): a launch only a few rounds of
// resident tiles deep pays a tile LIFETIME for filling and draining the chip, and the lifetime is resident tiles / rate
// (Little) -- fewer resident tiles at the same rate shorten it.  (Knobs build: HGI_DEC_WAVES / HGI_ENC_WAVES, tools/waves_sweep.sh.)
inline size_t lds_for_waves(size_t lds, int waves)
{
    if (waves <= 0) return lds;
    const size_t cap = ((size_t)160 * 1024 / (size_t)waves) & ~(size_t)255;
    return cap > lds ? cap : lds;
}

// How many tiles a CU holds at one time (the dynamic LDS is padded to that: lds_for_waves; 0: all its LDS allows, 32).  `tiles`:
// the launch's; `widest`: its widest row, pixels; `k`: the levels a tile fuses; `seeded`: the tiles start from a cone or from
// seed planes.
//  * Fewer than 8 192 tiles: all it can get -- the launch ends when its slowest wave does.
//  * A PLAIN decode (the tile holds the pyramid: no seeds) of 8 192 tiles and more: TEN on rows up to 4 096 pixels and up to
//    four levels, twelve otherwise.  Round 4, in-process A/B of builds on the same placed planes (tools/ab.py,
//    profiles/r04_ab_dec_waves.txt): 64 x 4096^2 level 4 against the 16 of the round's first builds: 9 tiles -1.9 %, 10 -5.2 %,
//    11 -3.1 %, 12 -0.8 %; 256 x -6.3 %, 512 x -5.5 % (2.789 -> 2.636 ms = 0.815 of 8 TB/s), 40 / 24 / 16 x -4.3 / -4.1 / -3.4 %,
//    8 x -0.8 %; levels 1 / 2 -1.4 / -2.1 %; 300 x 1920 x 1080 -2.3 %.  On 8192- and 16384-wide rows and at five levels twelve
//    is the better number (-2.8 / -2.3 ... -3.6 / -2.0 % against -2.4 / -0.6 ... -2.3 / -0.2 % at ten).  The likely reason:
//    with ten tiles per CU the 320 tiles an XCD has in flight read 2.7 MB at a time, which -- halo lines included -- stays in
//    its 4 MB L2; at 16 and more it does not (round 1 counted 1.06 x the algorithmic bytes fetched at 32); below ten the
//    latency is no longer covered.  At ONE level (the finest pass alone, P_fine) eight: 64 x 4096^2 0.3360 -> 0.3277 ms, 512 x
//    2.768 -> 2.692 (profiles/r04_ab_pfine.txt).
//  * A decode that rebuilds levels above its tiles (the cone) or starts from seed planes: 20 on launches one to eight
//    rounds of resident tiles deep (8 192 ... 65 536 tiles: a lone 16384^2 frame at level 8 has 32 768; the tile lifetime --
//    what filling and draining the chip costs -- is shorter at the same rate: 101.3 us at 32, 99.1 at 20, 98.5 at 16, 109.8
//    at 12, profiles/r03_waves_sweep.txt), 16 on deeper ones; these lose with ten or twelve (+3 ... +10 %: the cone's far
//    loads and its walk want the occupancy).  (The encoder needs all 20 it can get: 98 us, 106 at 16.)
// (Knobs build: HGI_DEC_WAVES forces a number for every launcher.)
inline int dec_resident_tiles(uint64_t tiles, uint32_t widest, uint32_t k, bool seeded)
{
    const int forced = HGI_KNOB(HGI_DEC_WAVES, -1);
    if (forced >= 0) return forced;
    if (tiles < 8192) return 0;
    if (!seeded) return widest > 4096 || k > 4 ? HGI_DEC_STREAM_WAVES_WIDE : k == 1 ? HGI_DEC_STREAM_WAVES_L1 : HGI_DEC_STREAM_WAVES;
    return tiles >= 65536 ? HGI_DEC_DEEP_WAVES : HGI_DEC_SHALLOW_WAVES;
}

}  // namespace hgi
