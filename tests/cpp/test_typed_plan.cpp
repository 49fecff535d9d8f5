// rustyhgi_amd/typed/hgi_typed_plan.h -- the two-sided plan of typed encode -- on random shapes, pitches,
// strides, addresses, batches and element sizes:
//   * every block of a launch walked through pitched_tile() (walk_launch, plan_test_util.h);
//   * `fast` against the documented rule evaluated here from scratch (include/hgi_typed.h): the image pitch and the grid pitch in
//     BYTES within the 32-bit bound, and -- 2-byte elements of an odd width -- the two bytes behind the last image frame's span
//     in the page of its last byte; fits32 / tail_ok say which half failed.  The GRID's address never enters: it is not read;
//   * on a fast plan every 32-bit offset the kernel forms -- the image side's (Y0 + 64 + 64) * pitch + (X0 + 128 + 64 + 16) * E,
//     the grid side's (Y0 + 63) * pitch + X0 + 128 for every block -- fits 32 bits when computed in 64; the write descriptor holds
//     exactly the grid span, the read descriptor the image span plus 0 or 2 bytes; every element of every row a tile loads
//     inside the image lies below the records;
// The byte intervals of the call, the page rule and the bound themselves are companion/hgi_sides.h's: test_sides.cpp.
// Usage: test_typed_plan [cases] [seed]
#include "../../rustyhgi_amd/typed/hgi_typed_plan.h"
#include "plan_test_util.h"

using namespace hgi;

namespace {

void plan_case(int i)
{
    TypedFrames f;
    const int kind = (int)(rnd() % 10);
    f.width = kind == 0 ? 1u : (uint32_t)rnd_in(1, kind < 7 ? 700 : 5000);
    f.height = kind == 1 ? 1u : (uint32_t)rnd_in(1, kind < 7 ? 400 : 3000);
    f.batch = (uint32_t)rnd_in(1, 4);
    f.elem = rnd() % 2 ? 2u : 4u;
    const uint32_t E = f.elem;
    const uint64_t gaps[] = {0, 1, 2, 3, 4, 16, 61, 128, 4096, 1u << 20, 1ull << 31, 1ull << 33};
    const int ng = kind == 9 ? 12 : 9;
    f.grid_pitch = f.width + gaps[rnd() % ng];
    f.img_pitch = ((uint64_t)f.width + gaps[rnd() % ng]) * E;      // gaps in elements
    if (rnd() % 5 == 0) {
        f.grid_pitch = f.width;
        f.img_pitch = (uint64_t)f.width * E;
    }
    const uint64_t row = (uint64_t)f.width * E;
    const uint64_t gp = f.height > 1 ? f.grid_pitch : f.width, ip = f.height > 1 ? f.img_pitch : row;
    const uint64_t gspan = pitched_span(f.width, f.height, gp), ispan = (uint64_t)(f.height - 1) * ip + row;
    f.grid_stride = gspan + (rnd() % 3 ? rnd_in(0, 300) : 0);
    f.img_stride = ispan + E * rnd_in(0, 150);
    uint64_t src = 0x7f0000000000ull + E * rnd_in(0, 1 << 19);
    if (rnd() % 3 == 0) {
        const uint64_t end = src + (uint64_t)(f.batch - 1) * (f.batch > 1 ? f.img_stride : 0) + ispan;
        src += (4096 - end % 4096) % 4096;      // ends on a page boundary
        src -= E * rnd_in(0, 2);
    }
    const TypedJudged j = typed_plan(src, f);
    const TypedPlan &r = j.plan;
    const PitchedPlan &p = r.p;
    const uint64_t tpf = (uint64_t)p.tx * p.ty;
    CHECK(p.ok, "case %d: plan refused", i);
    if (!p.ok) return;
    CHECK(p.tx == (f.width + 127) / 128 && p.ty == (f.height + 63) / 64, "case %d: tiles %u x %u", i, p.tx, p.ty);
    CHECK(p.dp == gp && j.ip == ip && j.ispan == ispan, "case %d: pitches", i);
    CHECK(p.dstride == (f.batch > 1 ? f.grid_stride : 0) && r.x.stride == (f.batch > 1 ? f.img_stride : 0), "case %d: strides", i);
    // the documented rule, from scratch
    const uint64_t end = src + (uint64_t)(f.batch - 1) * (f.batch > 1 ? f.img_stride : 0) + ispan;
    const bool fits = side_fits(f.height, gp) && side_fits(f.height, ip);
    const bool tail = E == 4 || f.width % 2 == 0 || end % 4096 != 0;
    CHECK(j.fits32 == fits, "case %d: fits32 %d, rule %d", i, (int)j.fits32, (int)fits);
    CHECK(j.tail_ok == tail, "case %d: tail_ok %d, rule %d", i, (int)j.tail_ok, (int)tail);
    CHECK((p.fast != 0) == (fits && tail), "case %d: fast %u, rule %d", i, p.fast, (int)(fits && tail));
    if (p.fast) {
        const uint64_t ymax = (uint64_t)(p.ty - 1) * 64 + 64 + 64, xmax = (uint64_t)(p.tx - 1) * 128 + 128 + 64 + 16;
        CHECK(ymax * gp + xmax < (1ull << 32), "case %d: grid side: 32-bit offset overflow (%llu rows, pitch %llu)", i,
              (unsigned long long)ymax, (unsigned long long)gp);
        CHECK(ymax * ip + xmax * E < (1ull << 32), "case %d: image side: 32-bit offset overflow (%llu rows, pitch %llu)", i,
              (unsigned long long)ymax, (unsigned long long)ip);
        CHECK(p.dp32 == gp && r.x.pitch32 == ip, "case %d: 32-bit pitches", i);
        CHECK(p.drec == gspan, "case %d: write records %u, span %llu", i, p.drec, (unsigned long long)gspan);
        CHECK(r.x.rec == ispan + (E == 2 && f.width % 2 ? 2 : 0), "case %d: read records %u, span %llu", i, r.x.rec, (unsigned long long)ispan);
        CHECK(ip % E == 0 && r.x.stride % E == 0 && src % E == 0, "case %d: whole elements", i);
    } else {
        // a refused plan describes no buffer path on either side
        CHECK(r.x.pitch32 == 0 && r.x.rec == 0 && p.dp32 == 0 && p.drec == 0 && p.ix == 0 && p.iy == 0 && p.nf == 0,
              "case %d: descriptors of a refused plan", i);
        return;     // nothing is launched
    }
    CHECK(p.nf == p.ipf * f.batch && p.nedge == (tpf - p.ipf) * f.batch && p.ipf == p.ix * p.iy, "case %d: totals", i);
    CHECK(p.ix == (f.width / 128) * (p.iy ? 1 : 0) && p.iy == (f.height / 64) * (p.ix ? 1 : 0), "case %d: interior %u x %u", i, p.ix, p.iy);
    // walk the launch: the tile's origin on both sides (bytes on the image side, pixels on the grid's)
    const WalkSide sides[2] = {{"grid", p.dp32, gp, 1}, {"image", r.x.pitch32, ip, E}};
    walk_launch(i, p, f.width, f.height, f.batch, sides, 2, [&](const PitchedTile &t, uint64_t b) {
        const uint32_t gbase = t.Y0 * p.dp32 + t.X0, ibase = t.Y0 * r.x.pitch32 + t.X0 * E;
        // the last row of the tile inside the image, its last element on both sides: the offsets fit 32 bits and lie below
        // the records (the image side's b128 load that holds the last element may reach the two tail bytes, never further)
        const uint32_t ylast = (t.Y0 + 63 < f.height ? t.Y0 + 63 : f.height - 1) - t.Y0;
        const uint32_t xend = (t.X0 + 128 < f.width ? t.X0 + 128 : f.width) - t.X0;
        const uint64_t glast = (uint64_t)gbase + (uint64_t)ylast * gp + xend, ilast = (uint64_t)ibase + (uint64_t)ylast * ip + (uint64_t)xend * E;
        CHECK(glast == (uint32_t)(gbase + ylast * p.dp32 + xend) && glast <= p.drec, "case %d: block %llu: last stored byte %llu, records %u", i,
              (unsigned long long)b, (unsigned long long)glast, p.drec);
        CHECK(ilast == (uint32_t)(ibase + ylast * r.x.pitch32 + xend * E) && ilast <= ispan, "case %d: block %llu: last loaded byte %llu, span %llu", i,
              (unsigned long long)b, (unsigned long long)ilast, (unsigned long long)ispan);
        // the dword that holds the last element of a row ends inside the records
        const uint64_t dw_end = ilast - E + 4 - ((ilast - E - ((uint64_t)ibase + (uint64_t)ylast * ip)) % 4);
        CHECK(dw_end <= r.x.rec, "case %d: block %llu: the last element's dword ends at %llu, records %u", i, (unsigned long long)b,
              (unsigned long long)dw_end, r.x.rec);
    });
}

}  // namespace

int main(int argc, char **argv)
{
    const int cases = argc > 1 ? std::atoi(argv[1]) : 300;
    if (argc > 2) g_x ^= std::strtoull(argv[2], nullptr, 0);
    for (int i = 0; i < cases; ++i) plan_case(i);
    {
        // the image side alone pushes the offsets past 32 bits: refused, never narrowed (4096 elements of 4 bytes, 2^18 apart)
        TypedFrames f = {4096u, 4096u, 2u, 4u, 1ull << 20, 4096, 1ull << 32, 1ull << 24};
        const TypedJudged r = typed_plan(0x7f0000000000ull, f);
        CHECK(r.plan.p.ok && !r.plan.p.fast && !r.fits32 && r.tail_ok && r.plan.x.pitch32 == 0 && r.plan.x.rec == 0 && r.plan.p.dp32 == 0 &&
                  r.plan.p.nf == 0, "a 2^20-byte image pitch on 4096 rows must be refused, on both sides");
        f.img_pitch = 1ull << 19;
        const TypedJudged q = typed_plan(0x7f0000000000ull, f);
        CHECK(q.plan.p.fast && q.fits32 && q.plan.x.pitch32 == (1u << 19), "a 2^19-byte image pitch on 4096 rows fits");
        // 2-byte elements, an odd width, the span of the last frame ending on the last byte of a page: two bytes more leave it
        TypedFrames g = {131u, 3u, 1u, 2u, 264, 131, 0, 0};
        const uint64_t span = 2 * 264 + 262;
        CHECK(!typed_plan(0x7f0000001000ull - span, g).plan.p.fast && !typed_plan(0x7f0000001000ull - span, g).tail_ok, "tail over a page end");
        CHECK(typed_plan(0x7f0000001000ull - span - 2, g).plan.p.fast && typed_plan(0x7f0000001000ull - span - 2, g).plan.x.rec == span + 2,
              "tail inside the page");
        CHECK(typed_plan(0x7f0000001000ull - span + 2, g).plan.p.fast, "tail at the start of the next page");
        g.elem = 4;      // 4-byte elements never read behind the span
        g.img_pitch = 528;
        CHECK(typed_plan(0x7f0000001000ull - (2 * 528 + 524), g).plan.p.fast && typed_plan(0x7f0000001000ull - (2 * 528 + 524), g).plan.x.rec == 2 * 528 + 524,
              "4-byte elements at a page end");
        g.elem = 2;      // an even width neither
        g.width = 130;
        g.img_pitch = 264;
        g.grid_pitch = 130;
        CHECK(typed_plan(0x7f0000001000ull - (2 * 264 + 260), g).plan.p.fast, "an even width at a page end");
        // the grid's width class does not matter: it is written, never read (widths 1, 2, 3 mod 4 at any image address)
        for (uint32_t w = 129; w < 133; ++w) {
            TypedFrames e = {w, 70u, 3u, 4u, 4ull * w + 12, w + 5, 70ull * (4 * w + 12), 70ull * (w + 5) + 1};
            for (uint64_t a = 0; a < 4096; a += 4) CHECK(typed_plan(0x7f0000000000ull + a, e).plan.p.fast, "width %u at image address +%llu", w, (unsigned long long)a);
        }
    }
    std::printf("%d cases, %d failures\n", cases, g_bad);
    return g_bad ? 1 : 0;
}
