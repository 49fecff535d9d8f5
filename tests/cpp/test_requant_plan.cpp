// rustyhgi_amd/requant/hgi_requant_plan.h -- the two-sided plan of requantize -- on random shapes,
// pitches, alignments and batches, against plain 64-bit arithmetic:
//   * every block of a launch walked through pitched_tile() (walk_launch, plan_test_util.h);
//   * `fast` against the documented rule evaluated here from scratch (include/hgi_requant.h): both pitches within the 32-bit
//     bound, and -- width % 4 != 0 -- the three bytes behind the last SOURCE frame's span in the page of its last byte;
//     fits32 / tail_ok say which half failed;
//   * on a fast plan every 32-bit offset the kernels form on both sides -- (Y0 + 64 + 64) * pitch + X0 + 128 + 64 + 16 -- fits
//     32 bits when computed in 64; the write descriptor holds exactly its span, the read descriptor the span plus 0 or 3 bytes;
//     a row at or below the image's height starts at or beyond the records on both sides;
// The byte intervals of the call, the page rule and the bound themselves are companion/hgi_sides.h's: test_sides.cpp.
// Usage: test_requant_plan [cases] [seed]
#include "../../rustyhgi_amd/requant/hgi_requant_plan.h"
#include "plan_test_util.h"

using namespace hgi;

namespace {

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
    // walk the launch: the tile's origin on the two sides
    const WalkSide sides[2] = {{"source", p.sp32, ip, 1}, {"destination", p.dp32, gp, 1}};
    walk_launch(i, p, f.width, f.height, f.batch, sides, 2);
}

}  // namespace

int main(int argc, char **argv)
{
    const int cases = argc > 1 ? std::atoi(argv[1]) : 300;
    if (argc > 2) g_x ^= std::strtoull(argv[2], nullptr, 0);
    for (int i = 0; i < cases; ++i) plan_case(i);
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
    }
    std::printf("%d cases, %d failures\n", cases, g_bad);
    return g_bad ? 1 : 0;
}
