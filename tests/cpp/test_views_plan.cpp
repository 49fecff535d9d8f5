// rustyhgi_amd/views/hgi_views_plan.h -- the host plan of the view lists -- under ASan / UBSan, a stand-alone program:
//   * block map: every block of random small lists (1 ... 40 entries, sides 0 ... 700, pitches w + {0, 1, 3, 16, 61, 128}) walked
//     through the functions the kernels run (list_role, list_find, view_tile): every tile of every non-empty frame exactly once,
//     ragged tiles first, idle blocks only in the padding to eight, interior tiles frame-major and row-major in contiguous
//     eighths, the found frame equal to a linear scan's; among them the special lists -- no edge tile at all, no interior tile at
//     all, fewer than eight interior tiles, one frame, frames without tiles of one kind between frames that have them;
//   * per-frame geometry: the record and the prefix sums against pitched_plan of a batch of one, field by field;
//   * aliasing: on random canvases of up to 96 x 48 bytes against a brute-force byte-set model -- same-pitch placements agree
//     exactly, both ways, one-row views against any pitch; span-meeting views of more than one row and different pitches are
//     refused; inputs overlapping inputs are accepted;
//   * boundary rules, both sides of each boundary: the page rule at every offset of the last byte in a page for width % 4 in
//     {1, 2, 3}; side_fits32 at its bound on each side; the tile-count bound in 64 bits, refused before anything is allocated.
// Nothing here touches frame memory.  Usage: test_views_plan [lists] [seed]
#include <cstring>
#include <set>

#include "../../rustyhgi_amd/views/hgi_views_plan.h"
#include "plan_test_util.h"

using namespace hgi;

namespace {

const uint32_t kGaps[6] = {0, 1, 3, 16, 61, 128};
int g_no_edge = 0, g_no_int = 0, g_few_int = 0, g_one = 0, g_repeat = 0;

bool tail_rule(const hgi_view_pair &v)      // include/hgi_views.h, restated
{
    if (v.width % 4 == 0) return true;
    const uint64_t end = v.src + (uint64_t)(v.height - 1) * (v.height > 1 ? v.src_pitch : v.width) + v.width;
    return ((end - 1) >> 12) == ((end + 2) >> 12);
}

uint32_t linear_find(const uint32_t *pre, uint32_t m, uint32_t t)
{
    uint32_t f = 0;
    for (uint32_t i = 0; i < m; ++i)
        if (pre[i] <= t) f = i;
    return f;
}

// mode 0: sides 0 ... 700; 1: whole tiles only; 2: no frame holds a whole tile; 3: fewer than eight interior tiles; 4: one frame;
// 5: frames with tiles of one kind only, alternating
void one_list(int c, int mode)
{
    const size_t n = mode == 4 ? 1 : (size_t)rnd_in(1, 40);
    std::vector<hgi_view_pair> v(n);
    uint64_t at = (1ull << 40) + rnd_in(0, 4095);
    for (size_t i = 0; i < n; ++i) {
        uint32_t w = (uint32_t)rnd_in(0, 700), h = (uint32_t)rnd_in(0, 700);
        if (mode == 1 || (mode == 5 && i % 2 == 0)) w = 128 * (uint32_t)rnd_in(1, 5), h = 64 * (uint32_t)rnd_in(1, 6);
        if (mode == 2 || (mode == 5 && i % 2 == 1)) (rnd_in(0, 1) ? w : h) = (uint32_t)rnd_in(1, 63);
        if (mode == 3) w = i < 2 ? 128 + (uint32_t)rnd_in(0, 127) : (uint32_t)rnd_in(1, 127), h = i < 2 ? 64 * (uint32_t)rnd_in(1, 3) : h;
        if (mode == 4 && (!w || !h)) w = h = 300;
        v[i].width = w;
        v[i].height = h;
        v[i].src_pitch = w + kGaps[rnd_in(0, 5)];
        v[i].dst_pitch = w + kGaps[rnd_in(0, 5)];
        v[i].src = at + rnd_in(0, 130);
        at = v[i].src + (uint64_t)h * v[i].src_pitch + 8 + rnd_in(0, 300);
        v[i].dst = at + rnd_in(0, 130);
        at = v[i].dst + (uint64_t)h * v[i].dst_pitch + 8 + rnd_in(0, 300);
    }
    std::vector<uint8_t> blob((size_t)views_blob_bytes(n) + 1, 0xAB);
    hgi_views_info info;
    memset(&info, 0x5A, sizeof(info));
    const ViewsJudged j = views_plan(v.data(), n, blob.data(), &info);
    size_t first_tail = n;
    for (size_t i = n; i-- > 0;)
        if (v[i].width && v[i].height && !tail_rule(v[i])) first_tail = i;
    if (first_tail < n) {
        CHECK(j.verdict == kViewsTail && j.a == first_tail, "list %d: tail rule of view %zu, verdict %d at %zu", c, first_tail, (int)j.verdict, j.a);
        CHECK(info.magic == 0x5A5A5A5Au && blob[0] == 0xAB, "list %d: a refused plan wrote something", c);
        return;
    }
    CHECK(j.verdict == kViewsOk, "list %d: verdict %d at %zu", c, (int)j.verdict, j.a);
    if (j.verdict != kViewsOk) return;
    CHECK(blob.back() == 0xAB && views_info_consistent(info), "list %d: blob size / info", c);
    const ViewArgs a = view_args(blob.data(), info);
    // geometry and prefix sums against pitched_plan of a batch of one
    std::vector<size_t> idx;
    for (size_t i = 0; i < n; ++i)
        if (v[i].width && v[i].height) idx.push_back(i);
    const uint32_t m = info.count;
    CHECK(m == idx.size(), "list %d: %u records, %zu non-empty views", c, m, idx.size());
    if (m != idx.size()) return;
    uint64_t ne = 0, ni = 0;
    uint32_t wmax = 0;
    std::vector<std::vector<uint8_t>> seen(m);
    bool had_e = false, gap_e = false, had_i = false, gap_i = false;
    for (uint32_t f = 0; f < m; ++f) {
        const hgi_view_pair &s = v[idx[f]];
        const PitchedFrames pf = {s.width, s.height, 1u, s.src_pitch, s.dst_pitch, 0, 0};
        const PitchedPlan p = pitched_plan(s.src, pf, false);
        ViewFrame F;
        memcpy(&F, a.frames + f, sizeof(F));
        CHECK(p.fast == 1 && p.ok, "list %d view %zu: an accepted view is not on the buffer path", c, idx[f]);
        CHECK(F.src == s.src && F.dst == s.dst && F.width == p.W && F.height == p.H && F.width == s.width && F.height == s.height, "list %d frame %u: record", c, f);
        CHECK(F.full_x == p.ix && F.full_y == p.iy && view_tiles_x(F.width) == p.tx && view_tiles_y(F.height) == p.ty, "list %d frame %u: tiles", c, f);
        CHECK(F.sp32 == p.sp32 && F.dp32 == p.dp32 && F.srec == p.srec && F.drec == p.drec && F.sp32 == p.sp && F.dp32 == p.dp, "list %d frame %u: sides", c, f);
        CHECK(memcmp(&F.fd_fx, &p.fd_ix, sizeof(FastDiv)) == 0, "list %d frame %u: divisor", c, f);
        CHECK(a.epre[f] == ne && a.ipre[f] == ni, "list %d frame %u: prefix", c, f);
        if (p.epf == 0 && had_e) gap_e = true;
        if (p.epf && gap_e) ++g_repeat, gap_e = false;
        if (p.ipf == 0 && had_i) gap_i = true;
        if (p.ipf && gap_i) ++g_repeat, gap_i = false;
        had_e = had_e || p.epf;
        had_i = had_i || p.ipf;
        ne += p.epf;
        ni += p.ipf;
        wmax = s.width > wmax ? s.width : wmax;
        seen[f].assign((size_t)p.tx * p.ty, 0);
    }
    CHECK(info.edge_tiles == ne && info.interior_tiles == ni && info.max_width == wmax, "list %d: totals", c);
    g_no_edge += ne == 0;
    g_no_int += ni == 0;
    g_few_int += ni > 0 && ni < 8;
    g_one += m == 1;
    // every block
    const uint64_t blocks = list_blocks(ne, ni), ne8 = (ne + 7u) & ~(uint64_t)7u;
    std::vector<uint8_t> seen_t((size_t)ni, 0);
    for (uint64_t b = 0; b < blocks; ++b) {
        const ListBlock r = view_block((uint32_t)b, a);
        CHECK(r.idle == (b >= ne && b < ne8), "list %d block %llu: idle %d", c, (unsigned long long)b, r.idle);
        if (r.idle) continue;
        CHECK(r.edge == (b < ne), "list %d block %llu: ragged tiles first", c, (unsigned long long)b);
        const uint32_t *pre = r.edge ? a.epre : a.ipre;
        const uint32_t lin = linear_find(pre, m, r.t);
        CHECK(r.frame == lin, "list %d block %llu: frame %u, linear scan %u", c, (unsigned long long)b, r.frame, lin);
        if (r.frame >= m) continue;
        ViewFrame F;
        memcpy(&F, a.frames + r.frame, sizeof(F));
        const uint32_t tx = view_tiles_x(F.width), ty = view_tiles_y(F.height);
        CHECK(r.tx < tx && r.ty < ty, "list %d block %llu: tile (%u, %u) outside frame %u", c, (unsigned long long)b, r.tx, r.ty, r.frame);
        if (r.tx >= tx || r.ty >= ty) continue;
        const bool interior = r.tx < F.full_x && r.ty < F.full_y;
        CHECK(interior == !r.edge, "list %d block %llu: interior %d in an edge block %d", c, (unsigned long long)b, interior, r.edge);
        if (r.edge) {
            CHECK(r.t == b, "list %d block %llu: edge position", c, (unsigned long long)b);
        } else {      // contiguous eighths, frame-major and row-major
            const uint32_t fb = (uint32_t)(b - ne8), x = fb & 7u;
            const uint32_t lo = list_range_first((uint32_t)ni, x), hi = x == 7 ? (uint32_t)ni : list_range_first((uint32_t)ni, x + 1);
            CHECK(r.t == lo + (fb >> 3) && r.t < hi, "list %d block %llu: eighth %u holds [%u, %u), position %u", c, (unsigned long long)b, x, lo, hi, r.t);
            CHECK(r.t - a.ipre[r.frame] == r.ty * F.full_x + r.tx, "list %d block %llu: row-major position", c, (unsigned long long)b);
            if (r.t < ni) CHECK(seen_t[r.t]++ == 0, "list %d: interior position %u twice", c, r.t);
        }
        seen[r.frame][(size_t)r.ty * tx + r.tx]++;
    }
    for (uint32_t f = 0; f < m; ++f)
        for (size_t k = 0; k < seen[f].size(); ++k) CHECK(seen[f][k] == 1, "list %d frame %u tile %zu covered %u times", c, f, k, seen[f][k]);
    for (size_t t = 0; t < seen_t.size(); ++t) CHECK(seen_t[t] == 1, "list %d: interior position %zu not dealt", c, t);
    CHECK(view_block((uint32_t)blocks, a).idle, "list %d: the block behind the launch is idle", c);
}

// ---- aliasing against bytes -------------------------------------------------------------------------------------------------
struct Side {
    uint64_t p, pitch;      // pitch as given
    uint32_t w, h;
    size_t index;
    bool out;
    uint64_t eff() const { return h > 1 ? pitch : w; }
    uint64_t lo() const { return p; }
    uint64_t hi() const { return p + (uint64_t)(h - 1) * eff() + w; }
    bool holds(uint64_t a) const
    {
        if (a < p) return false;
        const uint64_t d = a - p, row = d / eff();
        return row < h && d % eff() < w;
    }
};

void one_canvas(int c)
{
    const uint32_t CP = (uint32_t)rnd_in(8, 96), CH = (uint32_t)rnd_in(2, 48);
    const uint64_t base = (1ull << 30) + 64, bytes = (uint64_t)CP * CH;
    const bool mixed = rnd_in(0, 3) == 0, in_only_overlap = rnd_in(0, 4) == 0;
    const size_t n = (size_t)rnd_in(1, mixed ? 3 : 5);
    std::vector<hgi_view_pair> v(n);
    std::vector<Side> sides;
    for (size_t i = 0; i < n; ++i) {
        const uint32_t w = (uint32_t)rnd_in(1, CP > 24 ? CP / 3 : CP), h = (uint32_t)rnd_in(1, CH > 9 ? CH / 3 : CH);
        uint64_t pitch[2], p[2];
        for (int o = 0; o < 2; ++o) {
            if (mixed && rnd_in(0, 1)) {      // a pitch of its own, anywhere in the canvas' bytes
                pitch[o] = w + rnd_in(0, 9);
                const uint64_t span = (uint64_t)(h - 1) * pitch[o] + w;
                p[o] = base + (span < bytes ? rnd_in(0, bytes - span) : 0);
            } else {                          // a window of the canvas
                pitch[o] = CP;
                p[o] = base + rnd_in(0, CH - h) * CP + rnd_in(0, CP - w);
            }
        }
        if (in_only_overlap) {                // outputs far away and apart: only inputs can meet
            pitch[1] = w;
            p[1] = (1ull << 40) + i * 65536;
        }
        v[i] = hgi_view_pair{p[0], p[1], w, h, pitch[0], pitch[1]};
        sides.push_back(Side{p[0], pitch[0], w, h, i, false});
        sides.push_back(Side{p[1], pitch[1], w, h, i, true});
    }
    // the model: a pair with an output in it is refused iff its spans meet and (the pitches differ or the byte sets meet)
    bool refuse = false, any_bytes = false, all_same = true;
    std::set<std::pair<size_t, size_t>> bad;      // (output's index, other's index), kind in the second's sign: out-out pairs both ways
    for (size_t x = 0; x < sides.size(); ++x)
        for (size_t y = x + 1; y < sides.size(); ++y) {
            const Side &s = sides[x], &t = sides[y];
            if (!s.out && !t.out) continue;
            bool share = false;
            for (uint64_t a = std::max(s.lo(), t.lo()); a < std::min(s.hi(), t.hi()) && !share; ++a) share = s.holds(a) && t.holds(a);
            const bool meet = s.lo() < t.hi() && t.lo() < s.hi();
            any_bytes = any_bytes || share;
            const bool differ = s.h > 1 && t.h > 1 && s.pitch != t.pitch;      // (a one-row view has no pitch to differ by)
            all_same = all_same && !differ;
            if (meet && (differ || share)) {
                refuse = true;
                bad.insert({s.out ? s.index : t.index, s.out ? t.index : s.index});
                if (s.out && t.out) bad.insert({t.index, s.index});
            }
        }
    std::vector<uint8_t> blob((size_t)views_blob_bytes(n));
    hgi_views_info info;
    const ViewsJudged j = views_plan(v.data(), n, blob.data(), &info);
    const bool refused = j.verdict == kViewsOutOut || j.verdict == kViewsOutIn;
    CHECK(j.verdict == kViewsOutOut || j.verdict == kViewsOutIn || j.verdict == kViewsOk || j.verdict == kViewsTail, "canvas %d: verdict %d", c, (int)j.verdict);
    CHECK(refused == refuse, "canvas %d (%zu views, mixed %d): refused %d, model %d", c, n, mixed, refused, refuse);
    if (all_same) CHECK(refused == any_bytes, "canvas %d: same pitches, refused %d, bytes shared %d", c, refused, any_bytes);
    if (in_only_overlap) CHECK(!refused, "canvas %d: inputs overlapping inputs were refused", c);
    if (refused && refuse) CHECK(bad.count({j.a, j.b}) == 1, "canvas %d: the pair %zu, %zu named is not an offending one", c, j.a, j.b);
}

// ---- boundaries ------------------------------------------------------------------------------------------------------------------
ViewsVerdict plan_of(const std::vector<hgi_view_pair> &v, hgi_views_info *info = nullptr)
{
    std::vector<uint8_t> blob((size_t)views_blob_bytes(v.size()));
    hgi_views_info mine;
    return views_plan(v.data(), v.size(), blob.data(), info ? info : &mine).verdict;
}

void boundaries()
{
    // the page rule: the last source byte at every offset of its page
    for (uint32_t m = 1; m <= 3; ++m)
        for (uint32_t off = 0; off < 4096; ++off) {
            const uint32_t w = 4 * (1 + off % 3) + m, h = 1 + off % 4;
            const uint64_t sp = w + kGaps[off % 6], span = (uint64_t)(h - 1) * sp + w;
            const uint64_t src = (7ull << 32) + 4096 * 4 + off + 1 - span;
            const std::vector<hgi_view_pair> v = {{1ull << 50, 2ull << 50, 8, 8, 8, 8}, {src, 1ull << 52, w, h, sp, (uint64_t)w + 3}};
            const ViewsVerdict got = plan_of(v);
            CHECK(got == (off + 3 <= 4095 ? kViewsOk : kViewsTail), "page rule: width %% 4 = %u, last byte at %u: verdict %d", m, off, (int)got);
        }
    {   // ... and a width that is a multiple of 4 is never asked
        const std::vector<hgi_view_pair> v = {{(7ull << 32) + 4096 - 12 * 3, 1ull << 52, 12, 3, 12, 12}};
        CHECK(plan_of(v) == kViewsOk, "page rule on dword rows");
    }
    // side_fits32 at its bound, on each side
    for (uint32_t h : {2u, 64u, 700u, 5000u}) {
        const uint64_t P = ((1ull << 32) - 1025) / ((uint64_t)h + 192);
        CHECK(side_fits32(h, P) && !side_fits32(h, P + 1), "bound of height %u", h);
        for (int side = 0; side < 2; ++side)
            for (int over = 0; over < 2; ++over) {
                hgi_view_pair e = {1ull << 50, 2ull << 50, 8, h, 8, 8};
                (side ? e.dst_pitch : e.src_pitch) = P + over;
                CHECK(plan_of({e}) == (over ? kViewsFits32 : kViewsOk), "32-bit bound: height %u side %d pitch %llu", h, side, (unsigned long long)(P + over));
            }
    }
    CHECK(plan_of({{1ull << 50, 2ull << 50, 8, 4, 1ull << 32, 8}}) == kViewsFits32, "a pitch of 2^32");
    CHECK(plan_of({{1ull << 50, 2ull << 50, 8, 1, 1ull << 40, 1ull << 63}}) == kViewsOk, "a one-row frame never steps by its pitch");
    // the tile-count bound, in 64 bits: 2^31 - 16 tiles pass it (and meet the 32-bit rule behind it), one more does not
    {
        const uint32_t W = 128u << 16, H = 64u * 32767u;
        std::vector<hgi_view_pair> v = {{1ull << 50, 1ull << 56, W, H, W, W}, {1ull << 58, 1ull << 59, 128u * (65536u - 16u), 1, 0, 0}};
        CHECK(list_tiles(W, H) + list_tiles(v[1].width, 1) == (1ull << 31) - 16, "tiles of the boundary list");
        CHECK(plan_of(v) == kViewsFits32, "2^31 - 16 tiles pass the tile rule");
        v.push_back({1ull << 60, 1ull << 61, 1, 1, 1, 1});
        hgi_views_info info;
        memset(&info, 0x5A, sizeof(info));
        CHECK(plan_of(v, &info) == kViewsTiles && info.magic == 0x5A5A5A5Au, "2^31 - 15 tiles");
        const std::vector<hgi_view_pair> one = {{1ull << 50, 1ull << 56, 0xFFFFFFFFu, 0xFFFFFFFFu, 1ull << 32, 1ull << 32}};
        CHECK(plan_of(one) == kViewsTiles, "one frame of 2^51 tiles");
        const std::vector<hgi_view_pair> many(3000, one[0]);      // the sum stays in 64 bits
        CHECK(plan_of(many) == kViewsTiles, "3000 frames of 2^51 tiles");
    }
    // rule order: the HGI_EINVAL rules first, in the header's order
    {
        hgi_view_pair ok = {1ull << 50, 2ull << 50, 30, 8, 40, 40};
        hgi_view_pair bad = ok;
        bad.src = 0;
        bad.src_pitch = 29;
        CHECK(plan_of({ok, bad}) == kViewsNullEntry, "NULL before pitch");
        bad = ok;
        bad.src_pitch = bad.dst_pitch = 29;
        CHECK(plan_of({bad}) == kViewsSrcPitch, "source pitch before destination pitch");
        bad = ok;
        bad.dst = bad.src;      // in place, and a side beyond 32 bits
        bad.dst_pitch = bad.src_pitch = 1ull << 33;
        CHECK(plan_of({bad}) == kViewsOutIn, "aliasing before the 32-bit rule");
        hgi_view_pair empty = {0, 0, 0, 9, 0, 0};
        hgi_views_info info;
        CHECK(plan_of({empty, empty}, &info) == kViewsOk && info.count == 0 && info.magic == HGI_VIEWS_MAGIC && views_info_consistent(info), "only empty entries");
        CHECK(plan_of({}, &info) == kViewsOk && info.count == 0 && views_info_consistent(info), "no entry");
        info.plan_bytes += 16;
        CHECK(!views_info_consistent(info), "a changed size is noticed");
    }
}

}  // namespace

int main(int argc, char **argv)
{
    const int cases = argc > 1 ? atoi(argv[1]) : 2000;
    if (argc > 2) g_x = strtoull(argv[2], nullptr, 0) | 1u;
    for (int c = 0; c < cases; ++c) {
        one_list(c, c % 16 < 10 ? 0 : c % 16 - 9 < 6 ? c % 16 - 9 : 0);
        one_canvas(c);
    }
    boundaries();
    if (cases >= 100)
        CHECK(g_no_edge && g_no_int && g_few_int && g_one && g_repeat, "special lists met: no edge %d, no interior %d, nint < 8 %d, one frame %d, repeated prefix %d",
              g_no_edge, g_no_int, g_few_int, g_one, g_repeat);
    std::printf("views plan: %d cases, %d failures\n", cases, g_bad);
    return g_bad ? 1 : 0;
}
