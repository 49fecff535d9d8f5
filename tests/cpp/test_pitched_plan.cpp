// rustyhgi_amd/csrc/hgi_pitched.h -- the plan and the block -> tile map of the pitched launches -- on random shapes, pitches,
// alignments and batches:
//   * every block of a launch walked through pitched_tile(): every tile of every frame is covered exactly once, interior tiles
//     have their body inside the image, idle blocks appear only in the padding behind the ragged tiles;
//   * on the buffer path every 32-bit offset the kernels form -- (Y0 + 64 + 64) * pitch + X0 + 128 + 64 + 16 on either side --
//     fits 32 bits when computed in 64, the descriptors hold exactly the span (write side) and the span plus 0 or 3 bytes (read
//     side), and the 3 bytes are granted only when the rows are not a multiple of 4 bytes, the bytes lie in the page of the
//     last frame's last byte and the frames in front of it are at least a span apart; a row at or below the image's height
//     starts at or beyond the records on both sides (it reads 0 and is dropped when stored);
//   * pitch == width on both sides reproduces fused_geom's result for the packed frame (restated here): the same fast bit, the
//     same interior tiles, the same tail.
// Shapes include 1 x 1, one-row frames with absurd pitches, widths 1 ... 3 mod 4, sources whose span ends 1 ... 3 bytes before
// a page end, pitches that push the offsets past 32 bits (metadata only: nothing here touches frame memory).
// Usage: test_pitched_plan [cases] [seed]
#include "../../rustyhgi_amd/csrc/hgi_pitched.h"
#include "plan_test_util.h"

using namespace hgi;

namespace {

// fused_geom (hgi_fused_impl.h), 128 x 64 tiles, no row limit, restated for a packed batch
struct Rule {
    bool fast, tail;
    uint32_t ix, iy;
};
Rule packed_rule(uint64_t src, uint32_t w, uint32_t h, uint32_t batch, uint64_t stride, bool force)
{
    Rule r;
    const uint64_t end = src + (uint64_t)(batch - 1) * stride + (uint64_t)w * h;
    const bool fits32 = ((uint64_t)h + 2 * 64 + 64) * w + 1024 < (1ull << 32);
    const bool tail_ok = (end - 1) / 4096 == (end + 2) / 4096 && (batch == 1 || stride >= (uint64_t)w * h);
    r.fast = fits32 && (w % 4 == 0 || tail_ok) && !force;
    r.tail = r.fast && w % 4 != 0;
    r.ix = r.fast ? w / 128 : 0;
    r.iy = r.fast ? h / 64 : 0;
    if (!r.ix || !r.iy) r.ix = r.iy = 0;
    return r;
}

void one_case(int i)
{
    PitchedFrames f;
    const int kind = (int)(rnd() % 10);
    f.width = kind == 0 ? 1u : (uint32_t)rnd_in(1, kind < 7 ? 700 : 5000);
    f.height = kind == 1 ? 1u : (uint32_t)rnd_in(1, kind < 7 ? 400 : 3000);
    f.batch = (uint32_t)rnd_in(1, 4);
    const uint64_t gaps[] = {0, 1, 2, 3, 4, 16, 61, 128, 4096, 1u << 20, 1ull << 31, 1ull << 33};
    f.src_pitch = f.width + gaps[rnd() % (kind == 9 ? 12 : 9)];
    f.dst_pitch = f.width + gaps[rnd() % (kind == 9 ? 12 : 9)];
    const bool same = rnd() % 5 == 0;
    if (same) f.src_pitch = f.dst_pitch = f.width;
    const uint64_t sspan = pitched_span(f.width, f.height, f.height > 1 ? f.src_pitch : f.width);
    const uint64_t dspan = pitched_span(f.width, f.height, f.height > 1 ? f.dst_pitch : f.width);
    f.src_stride = sspan + (rnd() % 3 ? rnd_in(0, 300) : 0);
    f.dst_stride = same && rnd() % 2 ? f.src_stride : dspan + rnd_in(0, 300);
    // the source: any alignment; every few cases the last frame's span ends 1 ... 3 bytes before a page end, or on it
    uint64_t src = 0x7f0000000000ull + rnd_in(0, 1 << 20);
    if (rnd() % 3 == 0) {
        const uint64_t end = src + (uint64_t)(f.batch - 1) * (f.batch > 1 ? f.src_stride : 0) + sspan;
        src += (4096 - end % 4096) % 4096;      // ends on a page boundary
        src -= rnd_in(0, 4);
    }
    const bool force = rnd() % 11 == 0;
    const PitchedPlan p = pitched_plan(src, f, force);
    const uint64_t tpf = (uint64_t)p.tx * p.ty;
    CHECK(p.tx == (f.width + 127) / 128 && p.ty == (f.height + 63) / 64, "case %d: tiles %u x %u", i, p.tx, p.ty);
    CHECK(p.ok, "case %d: plan refused", i);
    if (!p.ok) return;
    const uint64_t sp = f.height > 1 ? f.src_pitch : f.width, dp = f.height > 1 ? f.dst_pitch : f.width;
    CHECK(p.sp == sp && p.dp == dp, "case %d: pitches", i);
    CHECK(p.sstride == (f.batch > 1 ? f.src_stride : 0) && p.dstride == (f.batch > 1 ? f.dst_stride : 0), "case %d: strides", i);
    if (force) CHECK(!p.fast, "case %d: forced plan is fast", i);
    if (p.fast) {
        const uint64_t maxp = sp > dp ? sp : dp;
        // the deepest offsets: the last tile row's halo row 64 below the tile, the last tile column's halo column 64 + a chunk
        const uint64_t ymax = (uint64_t)(p.ty - 1) * 64 + 64 + 64, xmax = (uint64_t)(p.tx - 1) * 128 + 128 + 64 + 16;
        CHECK(ymax * maxp + xmax < (1ull << 32), "case %d: 32-bit offset overflow (%llu rows, pitch %llu)", i,
              (unsigned long long)ymax, (unsigned long long)maxp);
        CHECK(p.sp32 == sp && p.dp32 == dp, "case %d: 32-bit pitches", i);
        CHECK(p.drec == dspan, "case %d: write records %u, span %llu", i, p.drec, (unsigned long long)dspan);
        CHECK(p.srec == sspan || p.srec == sspan + 3, "case %d: read records %u, span %llu", i, p.srec, (unsigned long long)sspan);
        if (p.srec != sspan) {
            const uint64_t end = src + (uint64_t)(f.batch - 1) * p.sstride + sspan;
            CHECK(f.width % 4 != 0, "case %d: tail on dword rows", i);
            CHECK((end - 1) / 4096 == (end + 2) / 4096, "case %d: tail crosses a page", i);
            CHECK(f.batch == 1 || p.sstride >= sspan, "case %d: tail with overlapping frames", i);
        } else {
            CHECK(f.width % 4 == 0, "case %d: rows of %u bytes without the tail", i, f.width);
        }
        // a row at or below the image: its first byte is at or beyond the records (dwords that start there are out of range,
        // tail or not: start + 4 > span + 3)
        CHECK((uint64_t)f.height * sp >= sspan && (uint64_t)f.height * dp >= dspan, "case %d: row H inside the span", i);
    } else {
        CHECK(p.ix == 0 && p.iy == 0 && p.nf == 0, "case %d: interior tiles on the checked path", i);
    }
    if (f.src_pitch == f.width && f.dst_pitch == f.width && (f.batch == 1 || f.src_stride == f.dst_stride)) {
        const Rule r = packed_rule(src, f.width, f.height, f.batch, f.batch > 1 ? f.src_stride : (uint64_t)f.width * f.height, force);
        CHECK((p.fast != 0) == r.fast && p.ix == r.ix && p.iy == r.iy, "case %d: packed frame: fast %u/%d interior %u x %u / %u x %u", i,
              p.fast, (int)r.fast, p.ix, p.iy, r.ix, r.iy);
        if (p.fast) CHECK((p.srec == sspan + 3) == r.tail, "case %d: packed frame: tail", i);
    }
    CHECK(p.nf == p.ipf * f.batch && p.nedge == (tpf - p.ipf) * f.batch && p.ipf == p.ix * p.iy, "case %d: totals", i);
    walk_launch(i, p, f.width, f.height, f.batch, nullptr, 0);
}

}  // namespace

int main(int argc, char **argv)
{
    const int cases = argc > 1 ? std::atoi(argv[1]) : 300;
    if (argc > 2) g_x ^= std::strtoull(argv[2], nullptr, 0);
    for (int i = 0; i < cases; ++i) one_case(i);
    // shapes that do not fit one launch, or whose offsets leave 32 bits: refused / checked, never narrowed
    {
        PitchedFrames f = {70000u, 70000u, 1u, 1ull << 20, 70000u, 0, 0};
        const PitchedPlan p = pitched_plan(0x7f0000000000ull, f, false);
        CHECK(p.ok && !p.fast && p.nf == 0, "70000^2 at pitch 2^20 must take the checked path");
        PitchedFrames g = {4000000000u, 4000000000u, 1u, 4000000000ull, 4000000000ull, 0, 0};
        CHECK(!pitched_plan(0, g, false).ok, "a launch of 2^39 tiles must be refused");
        PitchedFrames e = {0u, 5u, 1u, 8, 8, 0, 0};
        CHECK(!pitched_plan(0, e, false).ok, "an empty frame has no launch");
    }
    std::printf("%d cases, %d failures\n", cases, g_bad);
    return g_bad ? 1 : 0;
}
