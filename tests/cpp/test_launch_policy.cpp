// rustyhgi_amd/csrc/hgi_launch_policy.h -- how many tiles of a decode a CU holds, for every decode launcher -- against a table
// written out here, and lds_for_waves at the LDS sizes around its cap.
//   * dec_resident_tiles at tiles in {1, 8191, 8192, 65535, 65536, 2^31}, widest row in {1, 4096, 4097}, k in {1, 2, 4, 5, 8},
//     unseeded and seeded: 0 below 8 192 tiles; unseeded 12 on rows wider than 4 096 or more than four levels, 8 at one level,
//     10 otherwise; seeded 20 below 65 536 tiles and 16 from there.
//   * lds_for_waves at 0, 8, 10, 12, 16, 20 and 32 waves for a request below and above the cap: never below the request; a
//     padded size is a multiple of 256 bytes, lets `waves` blocks into the 160 KiB of a CU and not one more.
// Built with -DHGI_DEC_STREAM_WAVES=9 (and EXPECT_STREAM=9) it shows that a build's own number reaches the rule.
// Usage: test_launch_policy
#include <cstdint>
#include <cstdio>

#include "../../rustyhgi_amd/csrc/hgi_launch_policy.h"

#ifndef EXPECT_STREAM
#define EXPECT_STREAM 10
#endif

namespace {

int failures = 0;

#define CHECK(cond, ...)                    \
    do {                                    \
        if (!(cond)) {                      \
            ++failures;                     \
            std::printf("FAIL %s: ", #cond); \
            std::printf(__VA_ARGS__);       \
            std::printf("\n");              \
        }                                   \
    } while (0)

const uint64_t kTiles[6] = {1, 8191, 8192, 65535, 65536, 1ull << 31};
const uint32_t kWidest[3] = {1, 4096, 4097};
const uint32_t kLevels[5] = {1, 2, 4, 5, 8};

// [seeded][tiles][widest][k]
const int kWant[2][6][3][5] = {
    {   // unseeded
        {{0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}},                                       // 1 tile
        {{0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}},                                       // 8 191
        {{8, EXPECT_STREAM, EXPECT_STREAM, 12, 12}, {8, EXPECT_STREAM, EXPECT_STREAM, 12, 12}, {12, 12, 12, 12, 12}},   // 8 192
        {{8, EXPECT_STREAM, EXPECT_STREAM, 12, 12}, {8, EXPECT_STREAM, EXPECT_STREAM, 12, 12}, {12, 12, 12, 12, 12}},   // 65 535
        {{8, EXPECT_STREAM, EXPECT_STREAM, 12, 12}, {8, EXPECT_STREAM, EXPECT_STREAM, 12, 12}, {12, 12, 12, 12, 12}},   // 65 536
        {{8, EXPECT_STREAM, EXPECT_STREAM, 12, 12}, {8, EXPECT_STREAM, EXPECT_STREAM, 12, 12}, {12, 12, 12, 12, 12}},   // 2^31
    },
    {   // seeded
        {{0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}},
        {{0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}},
        {{20, 20, 20, 20, 20}, {20, 20, 20, 20, 20}, {20, 20, 20, 20, 20}},
        {{20, 20, 20, 20, 20}, {20, 20, 20, 20, 20}, {20, 20, 20, 20, 20}},
        {{16, 16, 16, 16, 16}, {16, 16, 16, 16, 16}, {16, 16, 16, 16, 16}},
        {{16, 16, 16, 16, 16}, {16, 16, 16, 16, 16}, {16, 16, 16, 16, 16}},
    },
};

}  // namespace

int main()
{
    int cases = 0;
    for (int se = 0; se < 2; ++se)
        for (int t = 0; t < 6; ++t)
            for (int w = 0; w < 3; ++w)
                for (int k = 0; k < 5; ++k, ++cases) {
                    const int got = hgi::dec_resident_tiles(kTiles[t], kWidest[w], kLevels[k], se != 0);
                    CHECK(got == kWant[se][t][w][k], "tiles %llu widest %u k %u seeded %d: %d, want %d", (unsigned long long)kTiles[t],
                          kWidest[w], kLevels[k], se, got, kWant[se][t][w][k]);
                }
    const size_t cu = 160 * 1024;
    const int waves[7] = {0, 8, 10, 12, 16, 20, 32};
    for (int i = 0; i < 7; ++i) {
        const int n = waves[i];
        const size_t requests[4] = {256, 4848, cu / 32 + 16, cu / 8 + 4096};      // below every cap, k = 4's, above 32's, above every cap
        for (size_t req : requests) {
            const size_t got = hgi::lds_for_waves(req, n);
            ++cases;
            CHECK(got >= req, "waves %d request %zu: %zu is below the request", n, req, got);
            if (n == 0) {
                CHECK(got == req, "no number asked for, request %zu: %zu", req, got);
                continue;
            }
            if (got == req) {      // left alone: no multiple of 256 bytes above the request lets `n` blocks into a CU
                CHECK((req / 256 + 1) * 256 * (size_t)n > cu, "waves %d request %zu was not padded", n, req);
                continue;
            }
            CHECK(got % 256 == 0, "waves %d request %zu: %zu is not 256-byte granular", n, req, got);
            CHECK(got * (size_t)n <= cu, "waves %d request %zu: %d blocks of %zu bytes do not fit a CU", n, req, n, got);
            CHECK((got + 256) * (size_t)n > cu, "waves %d request %zu: %zu bytes could be 256 more", n, req, got);
        }
    }
    std::printf("%d cases, %d failures (plain decode of four levels: %d)\n", cases, failures, EXPECT_STREAM);
    return failures ? 1 : 0;
}
