// rustyhgi_amd/map/hgi_map_plan.h -- the two-sided plan of mapped decode -- on random shapes, pitches,
// alignments, batches and element sizes:
//   * every block of a launch walked through pitched_tile() (walk_launch, plan_test_util.h);
//   * `fast` against the documented rule evaluated here from scratch (include/hgi_map.h): the grid pitch and the output pitch in
//     BYTES within the 32-bit bound, and -- width % 4 != 0 -- the three bytes behind the last grid frame's span in the page of
//     its last byte; fits32 / tail_ok say which half failed;
//   * on a fast plan every 32-bit offset the kernel forms -- the grid side's (Y0 + 64 + 64) * pitch + X0 + 128 + 64 + 16, the
//     output side's (Y0 + 63) * pitch + (X0 + 128) * E for every block -- fits 32 bits when computed in 64; the write
//     descriptor holds exactly the output span, the read descriptor the grid span plus 0 or 3 bytes; every byte of every row a
//     tile stores inside the image lies below the records, and a row at or below the image's height starts at or beyond them;
// The byte intervals of the call, the page rule and the bound themselves are companion/hgi_sides.h's: test_sides.cpp.
// Usage: test_map_plan [cases] [seed]
#include "../../rustyhgi_amd/map/hgi_map_plan.h"
#include "plan_test_util.h"

using namespace hgi;

namespace {

void plan_case(int i)
{
    MapFrames f;
    const int kind = (int)(rnd() % 10);
    f.width = kind == 0 ? 1u : (uint32_t)rnd_in(1, kind < 7 ? 700 : 5000);
    f.height = kind == 1 ? 1u : (uint32_t)rnd_in(1, kind < 7 ? 400 : 3000);
    f.batch = (uint32_t)rnd_in(1, 4);
    f.elem = rnd() % 2 ? 2u : 4u;
    const uint32_t E = f.elem;
    const uint64_t gaps[] = {0, 1, 2, 3, 4, 16, 61, 128, 4096, 1u << 20, 1ull << 31, 1ull << 33};
    const int ng = kind == 9 ? 12 : 9;
    f.grid_pitch = f.width + gaps[rnd() % ng];
    f.out_pitch = ((uint64_t)f.width + gaps[rnd() % ng]) * E;      // gaps in elements
    if (rnd() % 5 == 0) {
        f.grid_pitch = f.width;
        f.out_pitch = (uint64_t)f.width * E;
    }
    const uint64_t row = (uint64_t)f.width * E;
    const uint64_t gp = f.height > 1 ? f.grid_pitch : f.width, op = f.height > 1 ? f.out_pitch : row;
    const uint64_t gspan = pitched_span(f.width, f.height, gp), ospan = (uint64_t)(f.height - 1) * op + row;
    f.grid_stride = gspan + (rnd() % 3 ? rnd_in(0, 300) : 0);
    f.out_stride = ospan + E * rnd_in(0, 150);
    uint64_t src = 0x7f0000000000ull + rnd_in(0, 1 << 20);
    if (rnd() % 3 == 0) {
        const uint64_t end = src + (uint64_t)(f.batch - 1) * (f.batch > 1 ? f.grid_stride : 0) + gspan;
        src += (4096 - end % 4096) % 4096;      // ends on a page boundary
        src -= rnd_in(0, 4);
    }
    const MapJudged j = map_plan(src, f);
    const MapPlan &r = j.plan;
    const PitchedPlan &p = r.p;
    const uint64_t tpf = (uint64_t)p.tx * p.ty;
    CHECK(p.ok, "case %d: plan refused", i);
    if (!p.ok) return;
    CHECK(p.tx == (f.width + 127) / 128 && p.ty == (f.height + 63) / 64, "case %d: tiles %u x %u", i, p.tx, p.ty);
    CHECK(p.sp == gp && j.op == op && j.ospan == ospan, "case %d: pitches", i);
    CHECK(p.sstride == (f.batch > 1 ? f.grid_stride : 0) && r.x.stride == (f.batch > 1 ? f.out_stride : 0), "case %d: strides", i);
    // the documented rule, from scratch
    const uint64_t end = src + (uint64_t)(f.batch - 1) * (f.batch > 1 ? f.grid_stride : 0) + gspan;
    const bool fits = side_fits(f.height, gp) && side_fits(f.height, op);
    const bool tail = f.width % 4 == 0 || (end - 1) / 4096 == (end + 2) / 4096;
    CHECK(j.fits32 == fits, "case %d: fits32 %d, rule %d", i, (int)j.fits32, (int)fits);
    CHECK(j.tail_ok == tail, "case %d: tail_ok %d, rule %d", i, (int)j.tail_ok, (int)tail);
    CHECK((p.fast != 0) == (fits && tail), "case %d: fast %u, rule %d", i, p.fast, (int)(fits && tail));
    if (p.fast) {
        const uint64_t ymax = (uint64_t)(p.ty - 1) * 64 + 64 + 64, xmax = (uint64_t)(p.tx - 1) * 128 + 128 + 64 + 16;
        CHECK(ymax * gp + xmax < (1ull << 32), "case %d: grid side: 32-bit offset overflow (%llu rows, pitch %llu)", i,
              (unsigned long long)ymax, (unsigned long long)gp);
        CHECK(ymax * op + xmax * E < (1ull << 32), "case %d: output side: 32-bit offset overflow (%llu rows, pitch %llu)", i,
              (unsigned long long)ymax, (unsigned long long)op);
        CHECK(p.sp32 == gp && r.x.pitch32 == op, "case %d: 32-bit pitches", i);
        CHECK(r.x.rec == ospan, "case %d: write records %u, span %llu", i, r.x.rec, (unsigned long long)ospan);
        CHECK(p.srec == gspan + (f.width % 4 ? 3 : 0), "case %d: read records %u, span %llu", i, p.srec, (unsigned long long)gspan);
        CHECK((uint64_t)f.height * gp >= gspan && (uint64_t)f.height * op >= ospan, "case %d: row H inside a span", i);
        CHECK(op % E == 0 && r.x.stride % E == 0, "case %d: whole elements", i);
    } else {
        // a refused plan describes no buffer path on either side
        CHECK(r.x.pitch32 == 0 && r.x.rec == 0 && p.sp32 == 0 && p.srec == 0 && p.ix == 0 && p.iy == 0 && p.nf == 0,
              "case %d: descriptors of a refused plan", i);
        return;     // nothing is launched
    }
    CHECK(p.nf == p.ipf * f.batch && p.nedge == (tpf - p.ipf) * f.batch && p.ipf == p.ix * p.iy, "case %d: totals", i);
    CHECK(p.ix == (f.width / 128) * (p.iy ? 1 : 0) && p.iy == (f.height / 64) * (p.ix ? 1 : 0), "case %d: interior %u x %u", i, p.ix, p.iy);
    // walk the launch: the tile's origin on both sides (pixels on the grid side, bytes on the output's)
    const WalkSide sides[2] = {{"grid", p.sp32, gp, 1}, {"output", r.x.pitch32, op, E}};
    walk_launch(i, p, f.width, f.height, f.batch, sides, 2, [&](const PitchedTile &t, uint64_t b) {
        const uint32_t obase = t.Y0 * r.x.pitch32 + t.X0 * E;
        // the last row the tile stores inside the image, its last element: the offset fits 32 bits and lies below the records;
        // the row below the image (if the tile reaches it) starts at or beyond them
        const uint32_t ylast = (t.Y0 + 63 < f.height ? t.Y0 + 63 : f.height - 1) - t.Y0;
        const uint32_t xend = (t.X0 + 128 < f.width ? t.X0 + 128 : f.width) - t.X0;
        const uint64_t last64 = (uint64_t)obase + (uint64_t)ylast * op + (uint64_t)xend * E;
        const uint32_t last32 = obase + ylast * r.x.pitch32 + xend * E;
        CHECK(last64 == last32 && last64 <= r.x.rec, "case %d: block %llu: last stored byte %llu, records %u", i, (unsigned long long)b,
              (unsigned long long)last64, r.x.rec);
        if (t.Y0 + 64 > f.height) {
            const uint64_t below = (uint64_t)f.height * op + (uint64_t)t.X0 * E;
            CHECK(below >= r.x.rec && below + 63 * op + 128 * E < (1ull << 32), "case %d: block %llu: a row below the image inside the records", i,
                  (unsigned long long)b);
        }
    });
}

}  // namespace

int main(int argc, char **argv)
{
    const int cases = argc > 1 ? std::atoi(argv[1]) : 300;
    if (argc > 2) g_x ^= std::strtoull(argv[2], nullptr, 0);
    for (int i = 0; i < cases; ++i) plan_case(i);
    {
        // the output side alone pushes the offsets past 32 bits: refused, never narrowed (4096 elements of 4 bytes, 2^18 apart)
        MapFrames f = {4096u, 4096u, 2u, 4u, 4096, 1ull << 20, 1ull << 24, 1ull << 32};
        const MapJudged r = map_plan(0x7f0000000000ull, f);
        CHECK(r.plan.p.ok && !r.plan.p.fast && !r.fits32 && r.tail_ok && r.plan.x.pitch32 == 0 && r.plan.x.rec == 0 && r.plan.p.sp32 == 0 &&
                  r.plan.p.nf == 0, "a 2^20-byte output pitch on 4096 rows must be refused, on both sides");
        f.out_pitch = 1ull << 19;
        const MapJudged q = map_plan(0x7f0000000000ull, f);
        CHECK(q.plan.p.fast && q.fits32 && q.plan.x.pitch32 == (1u << 19), "a 2^19-byte output pitch on 4096 rows fits");
        // the same grid fits at E = 2 and not at E = 4 when the packed output row is what crosses the bound
        MapFrames e = {1u << 19, 4096u, 1u, 2u, 1ull << 19, 1ull << 20, 0, 0};
        CHECK(!map_plan(0x7f0000000000ull, e).fits32, "4288 rows of 2^20 bytes do not fit");
        e.height = 3000;
        e.out_pitch = 1ull << 20;
        CHECK(map_plan(0x7f0000000000ull, e).fits32 && map_plan(0x7f0000000000ull, e).plan.p.fast, "3192 rows of 2^20 bytes fit");
        e.elem = 4;
        e.out_pitch = 1ull << 21;
        CHECK(!map_plan(0x7f0000000000ull, e).fits32, "3192 rows of 2^21 bytes do not fit");
        // the span of the last frame ends on the last byte of a page: three bytes more leave it
        MapFrames g = {130u, 3u, 1u, 2u, 130, 260, 0, 0};
        CHECK(!map_plan(0x7f0000001000ull - 390, g).plan.p.fast && !map_plan(0x7f0000001000ull - 390, g).tail_ok, "tail over a page end");
        CHECK(map_plan(0x7f0000001000ull - 394, g).plan.p.fast, "tail inside the page");
    }
    std::printf("%d cases, %d failures\n", cases, g_bad);
    return g_bad ? 1 : 0;
}
