// rustyhgi_amd/csrc/hgi_framelist.h -- the plan and the block -> tile map of the frame-list launches -- on random lists, every
// block of every launch walked through the functions the kernels run (list_role, list_find, list_tile):
//   * every tile of every frame is covered exactly once, and no block lands outside its frame's tile lattice;
//   * a tile is interior exactly when fused_geom's rule for a batch of one (restated here) makes it one, and each frame's
//     `aligned` bits are that rule's;
//   * idle blocks appear only in the padding behind the edge tiles;
//   * the frame search agrees with a linear scan, for every block and for random indices;
// and the overlap rule (list_overlap) agrees with an O(N^2) brute force.  Lists hold zero-size frames, 1 x 1 frames, widths
// 1 ... 3 mod 4, pointers at every alignment, frames whose last byte sits 1 ... 3 bytes before a page end and frames above
// 2^32 bytes (metadata only: nothing here touches frame memory).  Usage: test_framelist_plan [cases] [seed]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../rustyhgi_amd/csrc/hgi_framelist.h"

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
uint32_t rnd_in(uint32_t lo, uint32_t hi) { return lo + (uint32_t)(rnd() % ((uint64_t)hi - lo + 1)); }

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

// fused_geom (hgi_fused_impl.h) for a batch of one, 128 x 64 tiles, restated
struct Rule {
    bool fast;
    uint32_t ix, iy, aligned;
};
Rule rule(uint64_t src, uint64_t dst, uint32_t w, uint32_t h, bool force)
{
    Rule r;
    const uint64_t n = (uint64_t)w * h, end = src + n;
    const bool fits32 = ((uint64_t)h + 2 * 64 + 64) * w + 1024 < (1ull << 32);
    const bool tail_ok = (end - 1) / 4096 == (end + 2) / 4096;
    r.fast = fits32 && (w % 4 == 0 || tail_ok) && !force;
    r.ix = r.fast ? w / 128 : 0;
    r.iy = r.fast ? h / 64 : 0;
    if (!r.ix || !r.iy) r.ix = r.iy = 0;
    r.aligned = ((w % 16 == 0 && src % 16 == 0 && dst % 16 == 0) ? 1u : 0u) | (r.fast ? 2u : 0u) | (r.fast && w % 4 ? 4u : 0u);
    return r;
}

uint32_t linear_find(const std::vector<uint32_t> &pre, uint32_t t)
{
    uint32_t f = 0;
    for (uint32_t i = 0; i < pre.size(); ++i)
        if (pre[i] <= t) f = i;
    return f;
}

void one_list(size_t n, bool force, bool big)
{
    std::vector<uint64_t> src(n), dst(n);
    std::vector<uint32_t> w(n), h(n);
    uint64_t at = 1ull << 40;
    for (size_t i = 0; i < n; ++i) {
        const uint32_t kind = rnd_in(0, 9);
        if (kind == 0) {
            w[i] = rnd_in(0, 1) ? 0 : rnd_in(0, 300);
            h[i] = w[i] ? 0 : rnd_in(0, 300);
        } else if (kind == 1) {
            w[i] = h[i] = 1;
        } else if (kind == 2 && big) {          // above 2^32 bytes: the byte-checked path, metadata only
            w[i] = rnd_in(65536, 80000);
            h[i] = rnd_in(65537, 70000);
        } else {
            w[i] = rnd_in(1, 1400) * 4 + rnd_in(0, 3) * (rnd_in(0, 1));      // widths 0 ... 3 mod 4
            h[i] = rnd_in(1, 800);
            if (rnd_in(0, 3) == 0) w[i] = rnd_in(1, 20) * 128, h[i] = rnd_in(1, 12) * 64;   // whole tiles
        }
        const uint64_t bytes = (uint64_t)w[i] * h[i];
        src[i] = at + rnd_in(0, 63);                                      // every alignment
        if (rnd_in(0, 3) == 0 && bytes) {                                 // last byte 1 ... 3 (or 0, 4) bytes before a page end
            const uint64_t page_end = (src[i] + bytes + 4095) / 4096 * 4096 + 4096;
            src[i] = page_end - bytes - rnd_in(1, 5);
        }
        at = src[i] + bytes + rnd_in(0, 4096);
        dst[i] = at + rnd_in(0, 31);
        at = dst[i] + bytes + rnd_in(0, 4096);
    }
    std::vector<ListFrame> frames(n);
    std::vector<uint32_t> epre(n), ipre(n);
    uint32_t ne = 0, ni = 0;
    const uint32_t m = plan_list(src.data(), dst.data(), w.data(), h.data(), n, force, frames.data(), epre.data(), ipre.data(), &ne, &ni);
    frames.resize(m);
    epre.resize(m);
    ipre.resize(m);
    // the non-empty frames in list order, against the restated rule
    std::vector<size_t> idx;
    for (size_t i = 0; i < n; ++i)
        if (w[i] && h[i]) idx.push_back(i);
    CHECK(idx.size() == m, "%u frames planned, %zu non-empty", m, idx.size());
    if (idx.size() != m) return;
    uint64_t e_sum = 0, i_sum = 0;
    std::vector<std::vector<uint8_t>> seen(m);
    for (uint32_t f = 0; f < m; ++f) {
        const size_t i = idx[f];
        const ListFrame &F = frames[f];
        const Rule r = rule(src[i], dst[i], w[i], h[i], force);
        CHECK(F.src == src[i] && F.dst == dst[i] && F.width == w[i] && F.height == h[i], "frame %u record", f);
        CHECK(F.tiles_x == (w[i] + 127) / 128 && F.tiles_y == (h[i] + 63) / 64, "frame %u tiles", f);
        CHECK(F.full_x == r.ix && F.full_y == r.iy, "frame %u %ux%u interior %ux%u, rule %ux%u", f, w[i], h[i], F.full_x, F.full_y, r.ix, r.iy);
        CHECK(F.aligned == r.aligned, "frame %u aligned %u, rule %u", f, F.aligned, r.aligned);
        CHECK(epre[f] == e_sum && ipre[f] == i_sum, "frame %u prefix", f);
        e_sum += (uint64_t)F.tiles_x * F.tiles_y - (uint64_t)r.ix * r.iy;
        i_sum += (uint64_t)r.ix * r.iy;
        seen[f].assign((size_t)F.tiles_x * F.tiles_y, 0);
    }
    CHECK(ne == e_sum && ni == i_sum, "totals");
    ListArgs a = {frames.data(), epre.data(), ipre.data(), m, ne, ni};
    const uint64_t blocks = list_blocks(ne, ni);
    for (uint64_t b = 0; b < blocks; ++b) {
        const ListBlock r = list_block((uint32_t)b, a);
        const bool pad = b >= ne && b < ((ne + 7u) & ~7u);
        CHECK(r.idle == pad, "block %llu idle %d, padding %d", (unsigned long long)b, r.idle, pad);
        if (r.idle) continue;
        CHECK(r.edge == (b < ne), "block %llu kind", (unsigned long long)b);
        const std::vector<uint32_t> &pre = r.edge ? epre : ipre;
        CHECK(r.frame == linear_find(pre, r.t), "block %llu frame %u, linear scan %u", (unsigned long long)b, r.frame, linear_find(pre, r.t));
        if (r.frame >= m) continue;
        const ListFrame &F = frames[r.frame];
        CHECK(r.tx < F.tiles_x && r.ty < F.tiles_y, "block %llu tile (%u, %u) outside frame %u", (unsigned long long)b, r.tx, r.ty, r.frame);
        if (r.tx >= F.tiles_x || r.ty >= F.tiles_y) continue;
        const bool interior = r.tx < F.full_x && r.ty < F.full_y;
        CHECK(interior == !r.edge, "block %llu: tile (%u, %u) of frame %u interior %d, edge block %d", (unsigned long long)b, r.tx, r.ty,
              r.frame, interior, r.edge);
        seen[r.frame][(size_t)r.ty * F.tiles_x + r.tx]++;
    }
    CHECK(list_block((uint32_t)blocks, a).idle, "the block behind the launch is idle");
    for (uint32_t f = 0; f < m; ++f)
        for (size_t j = 0; j < seen[f].size(); ++j) CHECK(seen[f][j] == 1, "frame %u tile %zu covered %u times", f, j, seen[f][j]);
    // the search on its own: random indices, both arrays, and the clamp
    for (int k = 0; k < 200 && m; ++k) {
        const uint32_t te = ne ? rnd_in(0, ne - 1) : 0, ti = ni ? rnd_in(0, ni - 1) : 0;
        CHECK(list_find(epre.data(), m, te) == linear_find(epre, te), "edge search %u", te);
        CHECK(list_find(ipre.data(), m, ti) == linear_find(ipre, ti), "interior search %u", ti);
    }
    if (m) CHECK(list_find(epre.data(), m, 0xFFFFFFFFu) <= m - 1, "clamp");
}

// list_overlap against every pair
void one_overlap(size_t n)
{
    std::vector<ListSpan> spans;
    const uint64_t room = rnd_in(64, 4000);
    for (size_t i = 0; i < n; ++i) {
        for (int o = 0; o < 2; ++o) {
            const uint64_t lo = 4096 + rnd() % room, len = rnd_in(0, 3) == 0 ? 0 : rnd_in(1, 200);
            spans.push_back({lo, lo + len, i, o == 1});
        }
    }
    bool oo = false, oi = false;
    for (size_t x = 0; x < spans.size(); ++x)
        for (size_t y = x + 1; y < spans.size(); ++y) {
            const ListSpan &p = spans[x], &q = spans[y];
            if (p.hi <= p.lo || q.hi <= q.lo || !(p.lo < q.hi && q.lo < p.hi)) continue;
            if (p.out && q.out) oo = true;
            else if (p.out || q.out) oi = true;
        }
    std::vector<ListSpan> work = spans;
    size_t a = 0, b = 0;
    const int got = list_overlap(work, &a, &b);
    CHECK((got != 0) == (oo || oi), "overlap %d, brute force out/out %d out/in %d", got, oo, oi);
    if (got == 1) CHECK(oo, "reported two outputs meeting");
    if (!oo && oi) CHECK(got == 2, "only out/in pairs, got %d", got);
    if (oo && !oi) CHECK(got == 1, "only out/out pairs, got %d", got);
    if (got) {      // the pair named really meets
        bool found = false;
        for (const ListSpan &p : spans)
            for (const ListSpan &q : spans)
                if (p.index == a && q.index == b && p.out && q.out == (got == 1) && p.hi > p.lo && q.hi > q.lo && p.lo < q.hi && q.lo < p.hi &&
                    (&p != &q))
                    found = true;
        CHECK(found, "the pair %zu, %zu (kind %d) does not meet", a, b, got);
    }
}

}  // namespace

int main(int argc, char **argv)
{
    const int cases = argc > 1 ? atoi(argv[1]) : 300;
    if (argc > 2) g_x = strtoull(argv[2], nullptr, 0) | 1u;
    for (int c = 0; c < cases; ++c) {
        const size_t n = c % 10 == 0 ? 0 : c % 7 == 0 ? 1 : rnd_in(1, c % 3 == 0 ? 400 : 40);
        one_list(n, c % 5 == 4, c % 25 == 3);
        one_overlap(rnd_in(1, 60));
    }
    std::printf("framelist plan: %d cases, %d failures\n", cases, g_bad);
    return g_bad ? 1 : 0;
}
