// rustyhgi_amd/csrc/hgi_tilewalk.h -- the block -> tile walk of the uniform tile kernels -- walked on the CPU:
//   * exhaustively on small grids (0 ... 5 interior tile columns, 0 ... 20 interior tile rows, a ragged column and a ragged row
//     or none, batch 1 ... 10, bands of 1 ... 9 rows, both XCD dealings, forwards and backwards, and with the fast path off):
//     the non-idle blocks of a launch reach every (frame, tx, ty) exactly once; the idle blocks number ne8 - nedge and are the
//     last of the first ne8; interior blocks land on interior tiles and edge blocks on the others;
//   * the order promises of the header's comments: the list of interior tiles is band after band, column-major inside a band,
//     the last band of a frame taking the rows that are left; with xmode == 1 and sq < rr_own the eight blocks of one step sit
//     at the same offset of eight consecutive bands; with xmode == 0 block b takes range_first(nf, b & 7) + (b >> 3);
//     finish_grid clears xmode exactly when rem_rows != 0, when there are no interior tiles or when P == 0;
//   * on random large grids, up to the launchers' bound (all + 8 < 2^31 tiles), sampled blocks against a model that divides
//     with plain 64-bit arithmetic: the fast divisions by tpf, P, band, rem_rows (which may be 0) and ex.
// Usage: test_tilewalk [large grids] [seed]
//        test_tilewalk --census <file of "w h batch" lines> <tile height> <band> <xmode>     classes of the launches, one line
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#define HGI_TILE_ORDER 3      // the shipped order, as hgi_fused_dec.hip / hgi_fused_enc.hip set it
#include "../../rustyhgi_amd/csrc/hgi_tilewalk.h"

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

// fused_geom's tile lists (hgi_fused_impl.h) for ix x iy tiles inside the image plus the ragged ones, then finish_grid
TileGrid make_grid(uint32_t tiles_x, uint32_t tiles_y, uint32_t ix, uint32_t iy, uint32_t batch, uint32_t band, uint32_t xmode, uint32_t reverse)
{
    TileGrid g;
    std::memset(&g, 0, sizeof g);
    g.tiles_x = tiles_x;
    g.tiles_y = tiles_y;
    g.full_x = ix;
    g.full_y = iy;
    if (g.full_x == 0 || g.full_y == 0) g.full_x = g.full_y = 0;
    const uint64_t all = (uint64_t)tiles_x * tiles_y * batch, nfast = (uint64_t)g.full_x * g.full_y * batch;
    g.nfast = (uint32_t)nfast;
    g.nedge = (uint32_t)(all - nfast);
    g.reverse = reverse;
    g.band = band;
    g.xmode = xmode;
    finish_grid(g);
    return g;
}

struct Desc {
    uint32_t tiles_x, tiles_y, ix, iy, batch, band, xmode, reverse;
};
#define DESC_FMT "tiles %u x %u interior %u x %u batch %u band %u xmode %u reverse %u"
#define DESC_ARGS(d) d.tiles_x, d.tiles_y, d.ix, d.iy, d.batch, d.band, d.xmode, d.reverse

void check_finish(const TileGrid &g, const Desc &d)
{
    const bool keep = d.xmode == 1 && g.rem_rows == 0 && g.nf != 0 && g.P != 0;
    CHECK(g.xmode == (keep ? 1u : 0u), DESC_FMT ": xmode %u after finish_grid", DESC_ARGS(d), g.xmode);
    CHECK(g.nf == g.nfast && g.ex == g.full_x && g.tpf == g.full_x * g.full_y && g.P == g.band * g.full_x, DESC_FMT ": derived", DESC_ARGS(d));
    CHECK(g.band >= 1 && g.rem_rows == g.full_y % g.band && g.nfull == (g.full_y / g.band) * g.P, DESC_FMT ": bands", DESC_ARGS(d));
    if (g.xmode == 1) {
        const uint64_t nb = g.nf / g.P;
        CHECK((uint64_t)g.rr_own * 8 == (nb & ~7ull) * g.P && g.rr_tail0 == (nb & ~7ull) * g.P && g.rr_tail0 <= g.nf, DESC_FMT ": round-robin split", DESC_ARGS(d));
    } else {
        CHECK(g.rr_own == 0 && g.rr_tail0 == 0, DESC_FMT ": round-robin split without xmode 1", DESC_ARGS(d));
    }
}

// every block of the launch
void walk_launch(const Desc &d)
{
    const TileGrid g = make_grid(d.tiles_x, d.tiles_y, d.ix, d.iy, d.batch, d.band, d.xmode, d.reverse);
    check_finish(g, d);
    const uint32_t ne8 = (g.nedge + 7u) & ~7u, blocks = ne8 + g.nfast;
    const size_t tpf_all = (size_t)d.tiles_x * d.tiles_y;
    std::vector<uint8_t> seen(tpf_all * d.batch, 0);
    uint32_t idle = 0;
    for (uint32_t b = 0; b < blocks; ++b) {
        const BlockRole r = walk_block_role(b, g);
        CHECK(r.edge == (b < ne8), DESC_FMT ": block %u edge", DESC_ARGS(d), b);
        if (r.idle) {
            CHECK(b >= g.nedge && b < ne8, DESC_FMT ": idle block %u outside the padding", DESC_ARGS(d), b);
            ++idle;
            continue;
        }
        CHECK(!(b >= g.nedge && b < ne8), DESC_FMT ": block %u of the padding is not idle", DESC_ARGS(d), b);
        WalkTile t;
        if (r.edge) {
            CHECK(r.index == b, DESC_FMT ": edge block %u index %u", DESC_ARGS(d), b, r.index);
            t = walk_edge_tile(r.index, g);
        } else {
            const uint32_t fb = b - ne8, x = fb & 7u, sq = fb >> 3;
            CHECK(r.index < g.nf, DESC_FMT ": block %u position %u of %u", DESC_ARGS(d), b, r.index, g.nf);
            if (r.index >= g.nf) continue;
            if (g.xmode == 0) {
                CHECK(r.index == range_first(g.nf, x) + sq, DESC_FMT ": block %u: contiguous eighths", DESC_ARGS(d), b);
            } else if (sq < g.rr_own) {
                // the same offset of eight consecutive bands, the first of them a multiple of eight
                const uint32_t first = walk_block_role(ne8 + 8u * sq, g).index;
                CHECK(r.index == first + x * g.P && (first / g.P) % 8u == 0 && first % g.P == sq % g.P && first / g.P / 8u == sq / g.P,
                      DESC_FMT ": block %u: round-robin position %u, XCD 0 has %u", DESC_ARGS(d), b, r.index, first);
            } else {
                CHECK(r.index >= g.rr_tail0 && r.index == g.rr_tail0 + range_first(g.nf - g.rr_tail0, x) + (sq - g.rr_own),
                      DESC_FMT ": block %u: tail position %u", DESC_ARGS(d), b, r.index);
            }
            t = walk_fast_tile(walk_position(r.index, g), g);
        }
        const bool in_range = t.frame < d.batch && t.tx < d.tiles_x && t.ty < d.tiles_y;
        CHECK(in_range, DESC_FMT ": block %u -> frame %u tile (%u, %u)", DESC_ARGS(d), b, t.frame, t.tx, t.ty);
        if (!in_range) continue;
        const bool interior = t.tx < g.full_x && t.ty < g.full_y;
        CHECK(interior == !r.edge, DESC_FMT ": block %u (edge %d) on tile (%u, %u)", DESC_ARGS(d), b, (int)r.edge, t.tx, t.ty);
        uint8_t &s = seen[t.frame * tpf_all + (size_t)t.ty * d.tiles_x + t.tx];
        CHECK(s == 0, DESC_FMT ": tile (%u, %u) of frame %u covered twice", DESC_ARGS(d), t.tx, t.ty, t.frame);
        s = 1;
    }
    CHECK(idle == ne8 - g.nedge, DESC_FMT ": %u idle blocks", DESC_ARGS(d), idle);
    for (size_t k = 0; k < seen.size(); ++k) CHECK(seen[k] == 1, DESC_FMT ": tile %zu not covered", DESC_ARGS(d), k);
    // the band order itself: frame after frame, band after band, column after column, row after row
    uint32_t t = 0;
    for (uint32_t f = 0; f < d.batch && g.nf; ++f)
        for (uint32_t row0 = 0; row0 < g.full_y; row0 += g.band) {
            const uint32_t rows = g.full_y - row0 < g.band ? g.full_y - row0 : g.band;
            for (uint32_t tx = 0; tx < g.full_x; ++tx)
                for (uint32_t ty = row0; ty < row0 + rows; ++ty, ++t) {
                    const WalkTile w = walk_fast_tile(t, g);
                    CHECK(w.frame == f && w.tx == tx && w.ty == ty, DESC_FMT ": position %u is (%u, %u, %u), want (%u, %u, %u)", DESC_ARGS(d), t,
                          w.frame, w.tx, w.ty, f, tx, ty);
                }
        }
    CHECK(t == g.nf, DESC_FMT ": band order holds %u tiles of %u", DESC_ARGS(d), t, g.nf);
    if (g.nf) CHECK(walk_position(0, g) == (d.reverse ? g.nf - 1 : 0u) && walk_position(g.nf - 1, g) == (d.reverse ? 0u : g.nf - 1), DESC_FMT ": direction", DESC_ARGS(d));
}

uint64_t exhaustive()
{
    uint64_t n = 0;
    for (uint32_t ix = 0; ix <= 5; ++ix)
        for (uint32_t iy = 0; iy <= 20; ++iy)
            for (uint32_t rx = 0; rx <= 1; ++rx)
                for (uint32_t ry = 0; ry <= 1; ++ry) {
                    if (ix + rx == 0 || iy + ry == 0) continue;
                    for (uint32_t batch = 1; batch <= 10; ++batch) {
                        for (uint32_t band = 1; band <= 9; ++band)
                            for (uint32_t xmode = 0; xmode <= 1; ++xmode)
                                for (uint32_t reverse = 0; reverse <= 1; ++reverse, ++n)
                                    walk_launch(Desc{ix + rx, iy + ry, ix, iy, batch, band, xmode, reverse});
                        // the fast path off: every tile through the checked path (full_x = full_y = 0)
                        for (uint32_t xmode = 0; xmode <= 1; ++xmode, ++n) walk_launch(Desc{ix + rx, iy + ry, 0, 0, batch, 4, xmode, 0});
                    }
                }
    return n;
}

// ---- the model: plain 64-bit division
struct Model {
    bool edge, idle;
    uint64_t frame, tx, ty;
};
uint64_t eighth(uint64_t n, uint64_t x) { return x * (n / 8) + (x < n % 8 ? x : n % 8); }

Model model_block(uint64_t b, const Desc &d)
{
    const uint64_t fx = (d.ix && d.iy) ? d.ix : 0, fy = (d.ix && d.iy) ? d.iy : 0;
    const uint64_t all = (uint64_t)d.tiles_x * d.tiles_y * d.batch, nf = fx * fy * d.batch, nedge = all - nf, ne8 = (nedge + 7) / 8 * 8;
    Model m = {b < ne8, b < ne8 && b >= nedge, 0, 0, 0};
    if (m.idle) return m;
    if (m.edge) {
        const uint64_t right = (d.tiles_x - fx) * d.tiles_y, epf = right + fx * (d.tiles_y - fy);
        m.frame = b / epf;
        uint64_t i = b % epf;
        if (i < right) {
            m.ty = i / (d.tiles_x - fx);
            m.tx = fx + i % (d.tiles_x - fx);
        } else {
            i -= right;
            m.ty = fy + i / fx;
            m.tx = i % fx;
        }
        return m;
    }
    const uint64_t band = d.band < 1 ? 1 : d.band, P = band * fx, rem = fy % band, tpf = fx * fy, nfull = fy / band * P;
    const uint64_t fb = b - ne8, x = fb % 8, sq = fb / 8;
    uint64_t index;
    if (d.xmode == 1 && rem == 0) {
        const uint64_t nb8 = nf / P / 8 * 8, own = nb8 / 8 * P, tail0 = nb8 * P;
        index = sq < own ? (sq / P * 8 + x) * P + sq % P : tail0 + eighth(nf - tail0, x) + (sq - own);
    } else {
        index = eighth(nf, x) + sq;
    }
    const uint64_t t = d.reverse ? nf - 1 - index : index;
    m.frame = t / tpf;
    const uint64_t tt = t % tpf;
    if (tt < nfull) {
        const uint64_t r = tt % P;
        m.tx = r / band;
        m.ty = tt / P * band + r % band;
    } else {
        const uint64_t r = tt - nfull;
        m.tx = r / rem;
        m.ty = fy - rem + r % rem;
    }
    return m;
}

void large_case(int i)
{
    // a total of up to 2^31 - 9 tiles, split at random between columns, rows and frames
    Desc d;
    for (;;) {
        const double bits = 3.0 + (double)(rnd() % 28000) / 1000.0;
        const double a = (double)(rnd() % 1000) / 1000.0, b = (double)(rnd() % 1000) / 1000.0;
        const double lo = a < b ? a : b, hi = a < b ? b : a;
        d.ix = (uint32_t)(1ull << (unsigned)(bits * lo)) + (uint32_t)(rnd() % 3);
        d.iy = (uint32_t)(1ull << (unsigned)(bits * (hi - lo))) + (uint32_t)(rnd() % 3);
        d.batch = (uint32_t)(1ull << (unsigned)(bits * (1.0 - hi))) + (uint32_t)(rnd() % 3);
        d.ix = (uint32_t)rnd_in(d.ix / 2 + 1, d.ix);
        d.iy = (uint32_t)rnd_in(d.iy / 2 + 1, d.iy);
        d.tiles_x = d.ix + (uint32_t)(rnd() % 2);
        d.tiles_y = d.iy + (uint32_t)(rnd() % 2);
        if ((uint64_t)d.tiles_x * d.tiles_y * d.batch + 8 < (1ull << 31)) break;
    }
    switch (rnd() % 4) {
    case 0: d.band = (uint32_t)rnd_in(1, 9); break;
    case 1: d.band = (uint32_t)rnd_in(1, d.iy + 2); break;
    case 2: {      // a divisor of the rows: the round-robin arm
        d.band = (uint32_t)rnd_in(1, d.iy < 64 ? d.iy : 64);
        while (d.iy % d.band) --d.band;
        break;
    }
    default: d.band = 4; break;
    }
    d.xmode = (uint32_t)(rnd() % 3 ? 1 : 0);
    d.reverse = (uint32_t)(rnd() % 2);
    const TileGrid g = make_grid(d.tiles_x, d.tiles_y, d.ix, d.iy, d.batch, d.band, d.xmode, d.reverse);
    check_finish(g, d);
    const uint64_t ne8 = ((uint64_t)g.nedge + 7) & ~7ull, blocks = ne8 + g.nfast;
    CHECK(blocks < (1ull << 31), "case %d: %llu blocks", i, (unsigned long long)blocks);
    std::vector<uint64_t> bs;
    for (uint64_t k = 0; k < 16 && k < blocks; ++k) {
        bs.push_back(k);
        bs.push_back(blocks - 1 - k);
        if (ne8 + k < blocks) bs.push_back(ne8 + k);
        if (ne8 > k) bs.push_back(ne8 - 1 - k);
        const uint64_t turn = ne8 + 8ull * g.rr_own;      // where the round-robin part ends
        if (turn + k < blocks) bs.push_back(turn + k);
        if (turn > k) bs.push_back(turn - 1 - k);
    }
    for (int k = 0; k < 48; ++k) bs.push_back(rnd_in(0, blocks - 1));
    for (uint64_t b : bs) {
        const Model m = model_block(b, d);
        const BlockRole r = walk_block_role((uint32_t)b, g);
        CHECK(r.edge == m.edge && r.idle == m.idle, "case %d " DESC_FMT ": block %llu role", i, DESC_ARGS(d), (unsigned long long)b);
        if (r.idle || r.edge != m.edge) continue;
        if (!r.edge) CHECK(r.index < g.nf, "case %d " DESC_FMT ": block %llu position %u of %u", i, DESC_ARGS(d), (unsigned long long)b, r.index, g.nf);
        if (!r.edge && r.index >= g.nf) continue;
        const WalkTile t = r.edge ? walk_edge_tile(r.index, g) : walk_fast_tile(walk_position(r.index, g), g);
        CHECK(t.frame == m.frame && t.tx == m.tx && t.ty == m.ty, "case %d " DESC_FMT ": block %llu -> (%u, %u, %u), model (%llu, %llu, %llu)", i, DESC_ARGS(d),
              (unsigned long long)b, t.frame, t.tx, t.ty, (unsigned long long)m.frame, (unsigned long long)m.tx, (unsigned long long)m.ty);
    }
}

int census(const char *path, uint32_t th, uint32_t band, uint32_t xmode)
{
    std::FILE *f = std::fopen(path, "r");
    if (!f) return 2;
    unsigned w, h, batch;
    unsigned launches = 0, interior = 0, rr_tail = 0, rr_no_tail = 0, rr_none = 0, fallback_rem = 0, xmode0 = 0;
    std::set<uint32_t> rems;
    while (std::fscanf(f, "%u %u %u", &w, &h, &batch) == 3) {
        const TileGrid g = make_grid((w + 127) / 128, (h + th - 1) / th, w / 128, h / th, batch, band, xmode, 0);
        ++launches;
        if (!g.nf) continue;
        ++interior;
        if (g.rem_rows) rems.insert(g.rem_rows);
        if (g.xmode == 1) {
            if (g.rr_own == 0) ++rr_none;
            else if (g.rr_tail0 < g.nf) ++rr_tail;
            else ++rr_no_tail;
        } else {
            ++xmode0;
            if (xmode == 1 && g.rem_rows) ++fallback_rem;
        }
    }
    std::fclose(f);
    std::printf("launches=%u interior=%u rr_tail=%u rr_no_tail=%u rr_none=%u fallback_rem=%u xmode0=%u rem_rows=", launches, interior, rr_tail,
                rr_no_tail, rr_none, fallback_rem, xmode0);
    bool first = true;
    for (uint32_t r : rems) {
        std::printf("%s%u", first ? "" : ",", r);
        first = false;
    }
    std::printf("\n");
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc > 1 && !std::strcmp(argv[1], "--census")) {
        if (argc != 6) return 2;
        return census(argv[2], (uint32_t)std::atoi(argv[3]), (uint32_t)std::atoi(argv[4]), (uint32_t)std::atoi(argv[5]));
    }
    const int cases = argc > 1 ? std::atoi(argv[1]) : 20000;
    if (argc > 2) g_x ^= std::strtoull(argv[2], nullptr, 0);
    const uint64_t n = exhaustive();
    for (int i = 0; i < cases; ++i) large_case(i);
    std::printf("%llu small grids walked block by block, %d large grids sampled, %d failures\n", (unsigned long long)n, cases, g_bad);
    return g_bad ? 1 : 0;
}
