// rustyhgi_amd/companion/hgi_sides.h -- what the four companion libraries share on the host -- against brute force and at its
// boundaries:
//   * the byte intervals: three small layouts (rows of w, 2 w or 4 w bytes) and a table painted byte by byte into a
//     64-KiB arena -- an interval is exactly first byte to last byte, and two meet iff a byte of one lies between the first and
//     the last byte of the other; in place, one byte of overlap at either end, adjacency, an interval that wraps 64 bits;
//   * tail_in_page at each of the `extra` bytes in front of a page end, extra 2 and 3, one frame and several, and the rule
//     that the frames in front of the last are a span apart;
//   * side_fits32 at its boundary, side_span, split_levels and extra_side.
// Usage: test_sides [cases] [seed]
#include "../../rustyhgi_amd/companion/hgi_sides.h"
#include "plan_test_util.h"

using namespace hgi;

namespace {

// Sides 0 .. 2 with rows of w * E[k] bytes, side 3 a table of 256 * E[3] bytes.
void interval_case(int i)
{
    const uint32_t N = 1u << 16;
    const uint32_t w = (uint32_t)rnd_in(1, 40), h = (uint32_t)rnd_in(1, 12), batch = (uint32_t)rnd_in(1, 3);
    const uint32_t elems[3] = {1, 2, 4};
    Interval iv[4];
    std::vector<uint8_t> paint[4];
    uint64_t prev_ptr = 0, prev_total = 1;
    for (int k = 0; k < 4; ++k) {
        const uint32_t E = elems[rnd() % 3];
        const uint64_t row = (uint64_t)w * E;
        const uint64_t pitch = row + E * rnd_in(0, 30);
        const uint64_t span = (uint64_t)(h - 1) * pitch + row;
        const uint64_t stride = span + E * rnd_in(0, 50);
        const uint64_t total = k == 3 ? 256ull * E : (uint64_t)(batch - 1) * stride + span;
        // near or on one another every other case
        uint64_t ptr = k && rnd() % 2 ? prev_ptr + rnd_in(0, 2 * prev_total) : rnd_in(0, N - total - 1);
        if (ptr + total > N) ptr = N - total;
        iv[k] = k == 3 ? table_interval(ptr, 256ull * E) : side_interval(ptr, row, h, pitch, stride, batch);
        paint[k].assign(N, 0);
        uint64_t first = N, last = 0;
        if (k == 3) {
            first = ptr;
            last = ptr + 256ull * E - 1;
        } else {
            CHECK(side_span(row, h, pitch) == span, "interval %d side %d: span", i, k);
            for (uint32_t b = 0; b < batch; ++b)
                for (uint32_t y = 0; y < h; ++y)
                    for (uint64_t x = 0; x < row; ++x) {
                        const uint64_t a = ptr + b * stride + y * pitch + x;
                        first = a < first ? a : first;
                        last = a > last ? a : last;
                    }
        }
        for (uint64_t a = first; a <= last; ++a) paint[k][a] = 1;
        CHECK(iv[k].lo == first && iv[k].hi == last + 1, "interval %d side %d: [%llu, %llu) painted [%llu, %llu]", i, k,
              (unsigned long long)iv[k].lo, (unsigned long long)iv[k].hi, (unsigned long long)first, (unsigned long long)last);
        prev_ptr = ptr;
        prev_total = total;
    }
    for (int a = 0; a < 4; ++a)
        for (int b = a + 1; b < 4; ++b) {
            bool m = false;
            for (uint32_t j = 0; j < N && !m; ++j) m = paint[a][j] && paint[b][j];
            CHECK(meet(iv[a], iv[b]) == m && meet(iv[b], iv[a]) == m, "interval %d: sides %d / %d: meet %d", i, a, b, (int)m);
        }
}

// the page rule, from scratch: the last of the `extra` bytes behind `end` lies in the page of the byte in front of `end`
bool in_page(uint64_t end, uint32_t extra) { return (end - 1) / 4096 == (end - 1 + extra) / 4096; }

void tail_case(int i)
{
    const uint32_t E = rnd() % 2 ? 1u : 2u, extra = E == 1 ? 3u : 2u;      // the byte sides read 3 bytes behind, typed's 2-byte image 2
    const uint32_t w = (uint32_t)rnd_in(1, 300), h = rnd() % 4 ? (uint32_t)rnd_in(1, 40) : 1u, batch = (uint32_t)rnd_in(1, 4);
    const uint64_t row = (uint64_t)w * E, pitch = row + E * rnd_in(0, 64);
    const uint64_t span = (uint64_t)(h - 1) * (h > 1 ? pitch : row) + row;
    const bool apart = rnd() % 8 != 0;
    const uint64_t stride = apart ? span + E * rnd_in(0, 100) : rnd_in(0, span - 1);
    uint64_t first = 0x7f0000000000ull + E * rnd_in(0, 1 << 19);
    const uint64_t total = (uint64_t)(batch - 1) * (batch > 1 ? stride : 0) + span;
    if (rnd() % 2) first += (4096 - (first + total) % 4096) % 4096 - rnd_in(0, 5);      // ends within 5 bytes of a page end
    const bool want = in_page(first + total, extra) && (batch == 1 || stride >= span);
    CHECK(tail_in_page(first, row, h, pitch, stride, batch, extra) == want, "tail %d: %u x %u x %u rows of %llu, extra %u: rule %d", i, w, h, batch,
          (unsigned long long)row, extra, (int)want);
}

}  // namespace

int main(int argc, char **argv)
{
    const int cases = argc > 1 ? std::atoi(argv[1]) : 300;
    if (argc > 2) g_x ^= std::strtoull(argv[2], nullptr, 0);
    for (int i = 0; i < cases; ++i) interval_case(i);
    for (int i = 0; i < cases; ++i) tail_case(i);
    {
        // in place, one byte of overlap at either end, and adjacency
        const Interval a = side_interval(1000, 32, 8, 40, 320, 2);      // [1000, 1000 + 320 + 312)
        CHECK(a.hi - a.lo == 632, "span of two frames");
        CHECK(meet(a, a), "in place");
        CHECK(meet(a, side_interval(1631, 32, 8, 40, 320, 2)) && !meet(a, side_interval(1632, 32, 8, 40, 320, 2)), "the last byte");
        CHECK(meet(a, side_interval(1000 - 631, 32, 8, 40, 320, 2)) && !meet(a, side_interval(1000 - 632, 32, 8, 40, 320, 2)), "the first byte");
        // rows of elements: 32 elements of 4 bytes are 128 bytes
        CHECK(side_interval(1000, 128, 8, 160, 0, 1).hi == 1000 + 7 * 160 + 128, "rows of elements");
        // a single frame never steps by its stride
        CHECK(side_interval(1000, 32, 8, 40, 1 << 20, 1).hi == 1000 + 312, "one frame");
        // an interval that wraps 64 bits is representable (the callers refuse it by size)
        const Interval big = side_interval(~0ull - 10, 100, 1, 100, 0, 1);
        CHECK(big.hi > big.lo && big.hi - big.lo == 100, "128-bit interval");
        const Interval tb = table_interval(~0ull - 10, 1024);
        CHECK(tb.hi > tb.lo && tb.hi - tb.lo == 1024, "128-bit table interval");
        CHECK(meet(table_interval(500, 512), a) && !meet(table_interval(488, 512), a) && meet(table_interval(1631, 512), a) &&
                  !meet(table_interval(1632, 512), a), "the table at either end");
    }
    {
        // a frame of 3 rows of 130 bytes ending `back` bytes in front of a page end: the `extra` bytes behind it stay in the page
        // iff back >= extra
        const uint64_t page_end = 0x7f0000001000ull, span = 2 * 130 + 130;
        for (uint32_t extra = 2; extra <= 3; ++extra)
            for (uint64_t back = 0; back <= 4; ++back)
                CHECK(tail_in_page(page_end - span - back, 130, 3, 130, 0, 1, extra) == (back >= extra), "extra %u, %llu bytes in front of a page end", extra,
                      (unsigned long long)back);
        // ... the last of several frames is what counts, and the frames in front of it must be a span apart
        CHECK(!tail_in_page(page_end - 400 - span, 130, 3, 130, 400, 2, 3) && tail_in_page(page_end - 400 - span - 3, 130, 3, 130, 400, 2, 3), "two frames");
        CHECK(!tail_in_page(page_end - 389 - span - 3, 130, 3, 130, 389, 2, 3) && tail_in_page(page_end - 390 - span - 3, 130, 3, 130, 390, 2, 3),
              "frames closer than a span");
        // a one-row frame never steps by its pitch, a single frame never by its stride
        CHECK(tail_in_page(page_end - 130 - 3, 130, 1, 1 << 20, 5, 1, 3) && !tail_in_page(page_end - 130 - 2, 130, 1, 1 << 20, 5, 1, 3), "one row, one frame");
    }
    {
        // the bound: 4096 rows at 2^19 fit, at 2^20 they do not; a pitch of 2^32 never does; the boundary itself
        CHECK(side_fits32(4096, 1ull << 19) && !side_fits32(4096, 1ull << 20), "4096 rows at 2^19 / 2^20");
        const uint64_t most = ((1ull << 32) - 1025) / 193;      // the largest pitch with (1 + 192) * pitch + 1024 < 2^32
        CHECK(!side_fits32(1, 1ull << 32) && side_fits32(1, most) && !side_fits32(1, most + 1), "one row");
        for (int i = 0; i < cases; ++i) {
            const uint32_t h = (uint32_t)rnd_in(1, rnd() % 2 ? 5000 : 0xffffffffu);
            const uint64_t pitch = rnd_in(1, rnd() % 2 ? 1ull << 24 : 1ull << 33);
            CHECK(side_fits32(h, pitch) == side_fits(h, pitch), "bound at %u rows of %llu", h, (unsigned long long)pitch);
            // the largest offset of each user lies below the bound (hgi_sides.h lists them)
            if (side_fits32(h, pitch)) {
                const unsigned __int128 u8side = (unsigned __int128)(h + 128ull) * pitch + pitch + 208, mapped = (unsigned __int128)(h + 65ull) * pitch + 512,
                                        typed = (unsigned __int128)(h + 129ull) * pitch + 832;
                CHECK(u8side < (1ull << 32) && mapped < (1ull << 32) && typed < (1ull << 32), "offsets at %u rows of %llu", h, (unsigned long long)pitch);
            }
        }
    }
    {
        // csrc/hgi_capi.hip's split_pyramid, restated: up to five levels in the tile, six to eight as four under a cone
        const uint32_t want[9][2] = {{0, 0}, {1, 0}, {2, 0}, {3, 0}, {4, 0}, {5, 0}, {4, 2}, {4, 3}, {4, 4}};
        for (uint32_t l = 0; l <= 8; ++l) {
            uint32_t k = 99, up = 99;
            split_levels(l, &k, &up);
            CHECK(k == want[l][0] && up == want[l][1], "levels %u -> %u + %u", l, k, up);
        }
        const ExtraSide x = extra_side(true, 520, 4000, 77), y = extra_side(false, 520, 4000, 77);
        CHECK(x.pitch32 == 520 && x.rec == 4000 && x.stride == 77 && y.pitch32 == 0 && y.rec == 0 && y.stride == 77, "extra_side");
    }
    std::printf("%d cases, %d failures\n", cases, g_bad);
    return g_bad ? 1 : 0;
}
