// rustyhgi_amd/requant/hgi_requant_plan.h -- the two-sided plan of requantize and its interval test -- on random shapes,
// pitches, alignments and batches, against plain 64-bit arithmetic:
//   * every block of a launch walked through pitched_tile(): every tile of every frame covered exactly once, interior tiles with
//     their body inside the image, idle blocks only in the padding behind the ragged tiles;
//   * `fast` against the documented rule evaluated here from scratch (include/hgi_requant.h): both pitches within the 32-bit
//     bound, and -- width % 4 != 0 -- the three bytes behind the last SOURCE frame's span in the page of its last byte;
//     fits32 / tail_ok say which half failed;
//   * on a fast plan every 32-bit offset the kernels form on both sides -- (Y0 + 64 + 64) * pitch + X0 + 128 + 64 + 16 -- fits
//     32 bits when computed in 64; the write descriptor holds exactly its span, the read descriptor the span plus 0 or 3 bytes;
//     a row at or below the image's height starts at or beyond the records on both sides;
//   * the interval test against brute force: small layouts painted byte by byte into a map -- two sides meet iff a byte of one
//     lies between the first and the last byte of the other; in place and one-byte overlaps at either end are boundary cases.
// Usage: test_requant_plan [cases] [seed]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../rustyhgi_amd/requant/hgi_requant_plan.h"

using namespace hgi;

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

// the header's rule for one side, restated
bool side_fits(uint32_t h, uint64_t pitch) { return pitch < (1ull << 32) && ((uint64_t)h + 192) * pitch + 1024 < (1ull << 32); }

void plan_case(int i)
{
    RequantFrames f;
    const int kind = (int)(rnd() % 10);
    f.width = kind == 0 ? 1u : (uint32_t)rnd_in(1, kind < 7 ? 700 : 5000);
    f.height = kind == 1 ? 1u : (uint32_t)rnd_in(1, kind < 7 ? 400 : 3000);
    f.batch = (uint32_t)rnd_in(1, 4);
    const uint64_t gaps[] = {0, 1, 2, 3, 4, 16, 61, 128, 4096, 1u << 20, 1ull << 31, 1ull << 33};
    const int ng = kind == 9 ? 12 : 9;
    f.src_pitch = f.width + gaps[rnd() % ng];
    f.dst_pitch = f.width + gaps[rnd() % ng];
    if (rnd() % 5 == 0) f.src_pitch = f.dst_pitch = f.width;
    const uint64_t ip = f.height > 1 ? f.src_pitch : f.width, gp = f.height > 1 ? f.dst_pitch : f.width;
    const uint64_t ispan = pitched_span(f.width, f.height, ip), gspan = pitched_span(f.width, f.height, gp);
    f.src_stride = ispan + (rnd() % 3 ? rnd_in(0, 300) : 0);
    f.dst_stride = gspan + rnd_in(0, 300);
    uint64_t src = 0x7f0000000000ull + rnd_in(0, 1 << 20);
    if (rnd() % 3 == 0) {
        const uint64_t end = src + (uint64_t)(f.batch - 1) * (f.batch > 1 ? f.src_stride : 0) + ispan;
        src += (4096 - end % 4096) % 4096;      // ends on a page boundary
        src -= rnd_in(0, 4);
    }
    const RequantJudged j = requant_plan(src, f);
    const PitchedPlan &p = j.plan;
    const uint64_t tpf = (uint64_t)p.tx * p.ty;
    CHECK(p.ok, "case %d: plan refused", i);
    if (!p.ok) return;
    CHECK(p.tx == (f.width + 127) / 128 && p.ty == (f.height + 63) / 64, "case %d: tiles %u x %u", i, p.tx, p.ty);
    CHECK(p.sp == ip && p.dp == gp, "case %d: pitches", i);
    CHECK(p.sstride == (f.batch > 1 ? f.src_stride : 0) && p.dstride == (f.batch > 1 ? f.dst_stride : 0),
          "case %d: strides", i);
    // the documented rule, from scratch
    const uint64_t end = src + (uint64_t)(f.batch - 1) * (f.batch > 1 ? f.src_stride : 0) + ispan;
    const bool fits = side_fits(f.height, ip) && side_fits(f.height, gp);
    const bool tail = f.width % 4 == 0 || (end - 1) / 4096 == (end + 2) / 4096;
    CHECK(j.fits32 == fits, "case %d: fits32 %d, rule %d", i, (int)j.fits32, (int)fits);
    CHECK(j.tail_ok == tail, "case %d: tail_ok %d, rule %d", i, (int)j.tail_ok, (int)tail);
    CHECK((p.fast != 0) == (fits && tail), "case %d: fast %u, rule %d", i, p.fast, (int)(fits && tail));
    if (p.fast) {
        const uint64_t pitches[2] = {ip, gp};
        const uint64_t ymax = (uint64_t)(p.ty - 1) * 64 + 64 + 64, xmax = (uint64_t)(p.tx - 1) * 128 + 128 + 64 + 16;
        for (int s = 0; s < 2; ++s)
            CHECK(ymax * pitches[s] + xmax < (1ull << 32), "case %d: side %d: 32-bit offset overflow (%llu rows, pitch %llu)", i, s,
                  (unsigned long long)ymax, (unsigned long long)pitches[s]);
        CHECK(p.sp32 == ip && p.dp32 == gp, "case %d: 32-bit pitches", i);
        CHECK(p.drec == gspan, "case %d: write records %u", i, p.drec);
        CHECK(p.srec == ispan + (f.width % 4 ? 3 : 0), "case %d: read records %u, span %llu", i, p.srec, (unsigned long long)ispan);
        CHECK((uint64_t)f.height * ip >= ispan && (uint64_t)f.height * gp >= gspan,
              "case %d: row H inside a span", i);
    } else {
        // a refused plan describes no buffer path on either side
        CHECK(p.sp32 == 0 && p.dp32 == 0 && p.srec == 0 && p.drec == 0 && p.ix == 0 && p.iy == 0 && p.nf == 0,
              "case %d: descriptors of a refused plan", i);
        return;     // nothing is launched
    }
    CHECK(p.nf == p.ipf * f.batch && p.nedge == (tpf - p.ipf) * f.batch && p.ipf == p.ix * p.iy, "case %d: totals", i);
    CHECK(p.ix == (f.width / 128) * (p.iy ? 1 : 0) && p.iy == (f.height / 64) * (p.ix ? 1 : 0), "case %d: interior %u x %u", i, p.ix, p.iy);
    // walk the launch
    const uint64_t blocks = pitched_blocks(p);
    std::vector<uint8_t> seen((size_t)(tpf * f.batch), 0);
    uint64_t idle = 0;
    for (uint64_t b = 0; b < blocks; ++b) {
        const PitchedTile t = pitched_tile(p, (uint32_t)b);
        if (t.idle) {
            CHECK(b >= p.nedge && b < ((p.nedge + 7u) & ~7u), "case %d: idle block %llu outside the padding", i, (unsigned long long)b);
            ++idle;
            continue;
        }
        CHECK(t.frame < f.batch && t.X0 % 128 == 0 && t.Y0 % 64 == 0 && t.X0 < f.width && t.Y0 < f.height,
              "case %d: block %llu -> frame %u tile (%u, %u)", i, (unsigned long long)b, t.frame, t.X0, t.Y0);
        if (!(t.frame < f.batch && t.X0 < f.width && t.Y0 < f.height)) continue;
        const bool inside = (uint64_t)t.X0 + 128 <= f.width && (uint64_t)t.Y0 + 64 <= f.height;
        CHECK(t.edge != inside, "case %d: block %llu: edge %d, body inside %d", i, (unsigned long long)b, (int)t.edge, (int)inside);
        // the tile's origin and its last body row on the two sides, as the kernel forms them (32-bit arithmetic)
        const uint32_t bases[2] = {t.Y0 * p.sp32 + t.X0, t.Y0 * p.dp32 + t.X0};
        const uint64_t want[2] = {(uint64_t)t.Y0 * ip + t.X0, (uint64_t)t.Y0 * gp + t.X0};
        for (int s = 0; s < 2; ++s) CHECK(bases[s] == want[s], "case %d: side %d: tile origin wraps", i, s);
        uint8_t &s = seen[(size_t)(t.frame * tpf + (uint64_t)(t.Y0 / 64) * p.tx + t.X0 / 128)];
        CHECK(s == 0, "case %d: tile covered twice", i);
        s = 1;
    }
    CHECK(idle == ((p.nedge + 7u) & ~7u) - p.nedge, "case %d: %llu idle blocks", i, (unsigned long long)idle);
    for (size_t k = 0; k < seen.size(); ++k) CHECK(seen[k] == 1, "case %d: tile %zu not covered", i, k);
}

// Two small layouts somewhere in a 64-KiB arena; brute force: paint each side's conservative interval (first byte of the
// first frame to last byte of the last) and compare with requant_meet.
void interval_case(int i)
{
    const uint32_t N = 1u << 16;
    struct Side {
        uint64_t ptr, pitch, stride;
    } s[2];
    const uint32_t w = (uint32_t)rnd_in(1, 40), h = (uint32_t)rnd_in(1, 12), batch = (uint32_t)rnd_in(1, 3);
    RequantInterval iv[2];
    std::vector<uint8_t> paint[2];
    for (int k = 0; k < 2; ++k) {
        s[k].pitch = w + rnd_in(0, 30);
        const uint64_t span = (uint64_t)(h - 1) * s[k].pitch + w;
        s[k].stride = span + rnd_in(0, 50);
        const uint64_t total = (uint64_t)(batch - 1) * s[k].stride + span;
        // near or on one another every other case
        s[k].ptr = k && rnd() % 2 ? s[k - 1].ptr + rnd_in(0, 2 * total) : rnd_in(0, N - total - 1);
        if (s[k].ptr + total > N) s[k].ptr = N - total;
        iv[k] = requant_interval(s[k].ptr, w, h, s[k].pitch, s[k].stride, batch);
        paint[k].assign(N, 0);
        uint64_t first = N, last = 0;
        for (uint32_t b = 0; b < batch; ++b)
            for (uint32_t y = 0; y < h; ++y)
                for (uint32_t x = 0; x < w; ++x) {
                    const uint64_t a = s[k].ptr + b * s[k].stride + y * s[k].pitch + x;
                    first = a < first ? a : first;
                    last = a > last ? a : last;
                }
        for (uint64_t a = first; a <= last; ++a) paint[k][a] = 1;
        CHECK(iv[k].lo == first && iv[k].hi == last + 1, "interval %d side %d: [%llu, %llu) painted [%llu, %llu]", i, k,
              (unsigned long long)iv[k].lo, (unsigned long long)iv[k].hi, (unsigned long long)first, (unsigned long long)last);
    }
    for (int a = 0; a < 2; ++a)
        for (int b = a + 1; b < 2; ++b) {
            bool meet = false;
            for (uint32_t j = 0; j < N && !meet; ++j) meet = paint[a][j] && paint[b][j];
            CHECK(requant_meet(iv[a], iv[b]) == meet && requant_meet(iv[b], iv[a]) == meet, "interval %d: sides %d / %d: meet %d", i, a, b, (int)meet);
        }
}

}  // namespace

int main(int argc, char **argv)
{
    const int cases = argc > 1 ? std::atoi(argv[1]) : 300;
    if (argc > 2) g_x ^= std::strtoull(argv[2], nullptr, 0);
    for (int i = 0; i < cases; ++i) plan_case(i);
    for (int i = 0; i < cases; ++i) interval_case(i);
    {
        // the destination side alone pushes the offsets past 32 bits: refused, never narrowed
        RequantFrames f = {4096u, 4096u, 2u, 4096, 1ull << 20, 1ull << 24, 1ull << 32};
        const RequantJudged r = requant_plan(0x7f0000000000ull, f);
        CHECK(r.plan.ok && !r.plan.fast && !r.fits32 && r.tail_ok && r.plan.sp32 == 0 && r.plan.dp32 == 0 && r.plan.drec == 0 && r.plan.nf == 0,
              "a 2^20 destination pitch on 4096 rows must be refused, on both sides");
        f.dst_pitch = 1ull << 19;
        const RequantJudged q = requant_plan(0x7f0000000000ull, f);
        CHECK(q.plan.fast && q.fits32 && q.plan.dp32 == (1u << 19), "a 2^19 destination pitch on 4096 rows fits");
        // ... and so does the source side alone
        RequantFrames fs = {4096u, 4096u, 2u, 1ull << 20, 4096, 1ull << 32, 1ull << 24};
        CHECK(!requant_plan(0x7f0000000000ull, fs).plan.fast && !requant_plan(0x7f0000000000ull, fs).fits32, "a 2^20 source pitch on 4096 rows must be refused");
        // the span of the last source frame ends on the last byte of a page: three bytes more leave it
        RequantFrames g = {130u, 3u, 1u, 130, 130, 0, 0};
        CHECK(!requant_plan(0x7f0000001000ull - 390, g).plan.fast && !requant_plan(0x7f0000001000ull - 390, g).tail_ok, "tail over a page end");
        CHECK(requant_plan(0x7f0000001000ull - 394, g).plan.fast, "tail inside the page");
        for (uint64_t back = 391; back <= 393; ++back)
            CHECK(requant_plan(0x7f0000001000ull - back, g).tail_ok == (back == 393), "tail %llu bytes in front of a page end", (unsigned long long)back);
        // a multiple of 4 never asks
        RequantFrames g4 = {128u, 3u, 1u, 130, 130, 0, 0};
        CHECK(requant_plan(0x7f0000001000ull - (2 * 130 + 128), g4).plan.fast, "a width that is a multiple of 4 at a page end");
        // in place, one byte of overlap at either end, and adjacency
        const RequantInterval a = requant_interval(1000, 32, 8, 40, 320, 2);      // [1000, 1000 + 320 + 312)
        CHECK(a.hi - a.lo == 632, "span of two frames");
        CHECK(requant_meet(a, a), "in place");
        CHECK(requant_meet(a, requant_interval(1631, 32, 8, 40, 320, 2)) && !requant_meet(a, requant_interval(1632, 32, 8, 40, 320, 2)), "the last byte");
        CHECK(requant_meet(a, requant_interval(1000 - 631, 32, 8, 40, 320, 2)) && !requant_meet(a, requant_interval(1000 - 632, 32, 8, 40, 320, 2)), "the first byte");
        // an interval that wraps 64 bits is representable (the caller refuses it by size)
        const RequantInterval big = requant_interval(~0ull - 10, 100, 1, 100, 0, 1);
        CHECK(big.hi > big.lo && big.hi - big.lo == 100, "128-bit interval");
    }
    std::printf("%d cases, %d failures\n", cases, g_bad);
    return g_bad ? 1 : 0;
}
