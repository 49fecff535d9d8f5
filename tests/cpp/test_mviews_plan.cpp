// rustyhgi_amd/mviews/hgi_mviews_plan.h -- the host plan of the mapped view lists -- under ASan / UBSan, a stand-alone program:
//   * per-frame geometry: on random small lists (1 ... 40 entries, sides 0 ... 700, E in {2, 4}, grid pitches w + gap bytes, output
//     pitches (w + gap) * E bytes) the record and the prefix sums against pitched_plan of a batch of one on the grid side, the
//     written side in BYTES -- dp32 the byte pitch, drec the span (h - 1) * pitch + w * E -- field by field; every tile origin of the
//     written side formed in 32 bits as the kernel forms it equals the one formed in 64; every block of the launch walked through
//     view_block (the view lists' map, run unchanged): every tile of every non-empty frame exactly once;
//   * the output interval: dst_lo / dst_hi are the tight bounds of all output spans -- both are met by an output byte;
//   * aliasing: on random canvases of up to 192 x 48 bytes against a brute-force byte-set model with w * E bytes wide output
//     rectangles -- same-pitch placements agree exactly, both ways, one-row views against any pitch; span-meeting views of more
//     than one row and different pitches are refused; inputs overlapping inputs are accepted;
//   * boundary rules, both sides of each boundary: the page rule of the grid side at every offset of the last byte in a page;
//     side_fits32 at its bound on each side, the written side's in bytes; the element rules (dst and dst_pitch multiples of E,
//     dst_pitch >= w * E) at their bounds; the tile-count bound; the order of the rules; rows of 2^32 bytes and more.
// Nothing here touches frame memory.  Usage: test_mviews_plan [lists] [seed]
#include <cstring>
#include <set>

#include "../../rustyhgi_amd/mviews/hgi_mviews_plan.h"
#include "plan_test_util.h"

using namespace hgi;

namespace {

const uint32_t kGaps[6] = {0, 1, 3, 16, 61, 128};

bool tail_rule(const hgi_mview_pair &v)      // include/hgi_mviews.h, restated
{
    if (v.width % 4 == 0) return true;
    const uint64_t end = v.src + (uint64_t)(v.height - 1) * (v.height > 1 ? v.src_pitch : v.width) + v.width;
    return ((end - 1) >> 12) == ((end + 2) >> 12);
}

void one_list(int c)
{
    const uint32_t E = rnd_in(0, 1) ? 4 : 2;
    const size_t n = c % 16 == 15 ? 1 : (size_t)rnd_in(1, 40);
    std::vector<hgi_mview_pair> v(n);
    uint64_t at = (1ull << 40) + rnd_in(0, 4095);
    for (size_t i = 0; i < n; ++i) {
        uint32_t w = (uint32_t)rnd_in(0, 700), h = (uint32_t)rnd_in(0, 700);
        if (c % 16 == 14) w = 128 * (uint32_t)rnd_in(1, 5), h = 64 * (uint32_t)rnd_in(1, 6);
        v[i].width = w;
        v[i].height = h;
        v[i].src_pitch = w + kGaps[rnd_in(0, 5)];
        v[i].dst_pitch = (uint64_t)(w + kGaps[rnd_in(0, 5)]) * E;
        v[i].src = at + rnd_in(0, 130);
        at = v[i].src + (uint64_t)h * v[i].src_pitch + 8 + rnd_in(0, 300);
        v[i].dst = (at + rnd_in(0, 130) + E - 1) / E * E;
        at = v[i].dst + (uint64_t)h * v[i].dst_pitch + 8 + rnd_in(0, 300);
    }
    std::vector<uint8_t> blob((size_t)views_blob_bytes(n) + 1, 0xAB);
    hgi_mviews_info info;
    memset(&info, 0x5A, sizeof(info));
    const MViewsJudged j = mviews_plan(v.data(), n, E, blob.data(), &info);
    size_t first_tail = n;
    for (size_t i = n; i-- > 0;)
        if (v[i].width && v[i].height && !tail_rule(v[i])) first_tail = i;
    if (first_tail < n) {
        CHECK(j.verdict == kMViewsTail && j.a == first_tail, "list %d: tail rule of view %zu, verdict %d at %zu", c, first_tail, (int)j.verdict, j.a);
        CHECK(info.magic == 0x5A5A5A5Au && blob[0] == 0xAB, "list %d: a refused plan wrote something", c);
        return;
    }
    CHECK(j.verdict == kMViewsOk, "list %d: verdict %d at %zu", c, (int)j.verdict, j.a);
    if (j.verdict != kMViewsOk) return;
    CHECK(blob.back() == 0xAB && mviews_info_consistent(info) && info.elem_size == E, "list %d: blob size / info", c);
    const ViewArgs a = mview_args(blob.data(), info);
    std::vector<size_t> idx;
    for (size_t i = 0; i < n; ++i)
        if (v[i].width && v[i].height) idx.push_back(i);
    const uint32_t m = info.count;
    CHECK(m == idx.size(), "list %d: %u records, %zu non-empty views", c, m, idx.size());
    if (m != idx.size()) return;
    uint64_t ne = 0, ni = 0, lo = ~0ull, hi = 0;
    uint32_t wmax = 0;
    std::vector<std::vector<uint8_t>> seen(m);
    for (uint32_t f = 0; f < m; ++f) {
        const hgi_mview_pair &s = v[idx[f]];
        // the grid side: pitched_plan of a batch of one, its write side mirroring the read side (as map_plan makes it)
        const PitchedFrames pf = {s.width, s.height, 1u, s.src_pitch, s.src_pitch, 0, 0};
        const PitchedPlan p = pitched_plan(s.src, pf, false);
        // the written side in bytes
        const uint64_t op = s.height > 1 ? s.dst_pitch : (uint64_t)s.width * E, ospan = (uint64_t)(s.height - 1) * op + (uint64_t)s.width * E;
        ViewFrame F;
        memcpy(&F, a.frames + f, sizeof(F));
        CHECK(p.fast == 1 && p.ok, "list %d view %zu: an accepted view is not on the buffer path", c, idx[f]);
        CHECK(F.src == s.src && F.dst == s.dst && F.width == p.W && F.height == p.H && F.width == s.width && F.height == s.height, "list %d frame %u: record", c, f);
        CHECK(F.full_x == p.ix && F.full_y == p.iy && view_tiles_x(F.width) == p.tx && view_tiles_y(F.height) == p.ty, "list %d frame %u: tiles", c, f);
        CHECK(F.sp32 == p.sp32 && F.srec == p.srec && F.sp32 == p.sp, "list %d frame %u: grid side", c, f);
        CHECK(F.dp32 == op && F.drec == ospan, "list %d frame %u: written side %u / %u, want %llu / %llu", c, f, F.dp32, F.drec, (unsigned long long)op,
              (unsigned long long)ospan);
        CHECK(memcmp(&F.fd_fx, &p.fd_ix, sizeof(FastDiv)) == 0, "list %d frame %u: divisor", c, f);
        CHECK(a.epre[f] == ne && a.ipre[f] == ni, "list %d frame %u: prefix", c, f);
        ne += p.epf;
        ni += p.ipf;
        wmax = s.width > wmax ? s.width : wmax;
        lo = s.dst < lo ? s.dst : lo;
        hi = s.dst + ospan > hi ? s.dst + ospan : hi;
        seen[f].assign((size_t)p.tx * p.ty, 0);
    }
    CHECK(info.edge_tiles == ne && info.interior_tiles == ni && info.max_width == wmax, "list %d: totals", c);
    if (m == 0) lo = hi = 0;      // a plan of no frame has no output
    CHECK(info.dst_lo == lo && info.dst_hi == hi, "list %d: output interval [%llx, %llx), want [%llx, %llx)", c, (unsigned long long)info.dst_lo,
          (unsigned long long)info.dst_hi, (unsigned long long)lo, (unsigned long long)hi);
    // every block, through the view lists' map; the written side's tile origin in 32 bits
    const uint64_t blocks = list_blocks(ne, ni), ne8 = (ne + 7u) & ~(uint64_t)7u;
    for (uint64_t b = 0; b < blocks; ++b) {
        const ListBlock r = view_block((uint32_t)b, a);
        CHECK(r.idle == (b >= ne && b < ne8), "list %d block %llu: idle %d", c, (unsigned long long)b, r.idle);
        if (r.idle || r.frame >= m) continue;
        ViewFrame F;
        memcpy(&F, a.frames + r.frame, sizeof(F));
        const uint32_t tx = view_tiles_x(F.width), ty = view_tiles_y(F.height);
        CHECK(r.tx < tx && r.ty < ty, "list %d block %llu: tile (%u, %u) outside frame %u", c, (unsigned long long)b, r.tx, r.ty, r.frame);
        if (r.tx >= tx || r.ty >= ty) continue;
        CHECK((r.tx < F.full_x && r.ty < F.full_y) == !r.edge, "list %d block %llu: kind", c, (unsigned long long)b);
        const uint32_t X0 = r.tx * 128, Y0 = r.ty * 64, base = Y0 * F.dp32 + X0 * E;
        CHECK(base == (uint64_t)Y0 * F.dp32 + (uint64_t)X0 * E, "list %d block %llu: the written side's tile origin wraps", c, (unsigned long long)b);
        // the largest offset the mapped finest pass forms on the written side (companion/hgi_sides.h) stays in 32 bits
        CHECK((uint64_t)(Y0 + 64) * F.dp32 + (uint64_t)(X0 + 128) * E < (1ull << 32), "list %d block %llu: written side beyond 32 bits", c, (unsigned long long)b);
        seen[r.frame][(size_t)r.ty * tx + r.tx]++;
    }
    for (uint32_t f = 0; f < m; ++f)
        for (size_t k = 0; k < seen[f].size(); ++k) CHECK(seen[f][k] == 1, "list %d frame %u tile %zu covered %u times", c, f, k, seen[f][k]);
}

// ---- aliasing against bytes -------------------------------------------------------------------------------------------------
struct Side {
    uint64_t p, pitch;      // pitch as given, bytes
    uint64_t w;             // bytes of a row
    uint32_t h;
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
    const uint32_t E = rnd_in(0, 1) ? 4 : 2;
    const uint32_t CP = E * (uint32_t)rnd_in(8, 48), CH = (uint32_t)rnd_in(2, 48);      // the canvas' rows: whole elements
    const uint64_t base = (1ull << 30) + 64, bytes = (uint64_t)CP * CH;
    const bool mixed = rnd_in(0, 3) == 0, in_only_overlap = rnd_in(0, 4) == 0;
    const size_t n = (size_t)rnd_in(1, mixed ? 3 : 5);
    std::vector<hgi_mview_pair> v(n);
    std::vector<Side> sides;
    for (size_t i = 0; i < n; ++i) {
        const uint32_t we = CP / E;      // the canvas' width in elements
        const uint32_t w = (uint32_t)rnd_in(1, we > 12 ? we / 3 : we), h = (uint32_t)rnd_in(1, CH > 9 ? CH / 3 : CH);
        uint64_t pitch[2], p[2];
        for (int o = 0; o < 2; ++o) {
            const uint32_t e = o ? E : 1;      // the output is placed on whole elements
            if (mixed && rnd_in(0, 1)) {       // a pitch of its own, anywhere in the canvas' bytes
                pitch[o] = (uint64_t)(w + rnd_in(0, 9)) * e;
                const uint64_t span = (uint64_t)(h - 1) * pitch[o] + (uint64_t)w * e;
                p[o] = base + (span < bytes ? rnd_in(0, (bytes - span) / e) * e : 0);
            } else {                           // a window of the canvas
                pitch[o] = CP;
                p[o] = base + rnd_in(0, CH - h) * CP + rnd_in(0, (CP - w * e) / e) * e;
            }
        }
        if (in_only_overlap) {                 // outputs far away and apart: only inputs can meet
            pitch[1] = (uint64_t)w * E;
            p[1] = (1ull << 40) + i * 65536;
        }
        v[i] = hgi_mview_pair{p[0], p[1], w, h, pitch[0], pitch[1]};
        sides.push_back(Side{p[0], pitch[0], w, h, i, false});
        sides.push_back(Side{p[1], pitch[1], (uint64_t)w * E, h, i, true});
    }
    // the model: a pair with an output in it is refused iff its spans meet and (the pitches differ or the byte sets meet)
    bool refuse = false, any_bytes = false, all_same = true;
    std::set<std::pair<size_t, size_t>> bad;
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
    hgi_mviews_info info;
    const MViewsJudged j = mviews_plan(v.data(), n, E, blob.data(), &info);
    const bool refused = j.verdict == kMViewsOutOut || j.verdict == kMViewsOutIn;
    CHECK(refused || j.verdict == kMViewsOk || j.verdict == kMViewsTail, "canvas %d: verdict %d", c, (int)j.verdict);
    CHECK(refused == refuse, "canvas %d (%zu views, E %u, mixed %d): refused %d, model %d", c, n, E, mixed, refused, refuse);
    if (all_same) CHECK(refused == any_bytes, "canvas %d: same pitches, refused %d, bytes shared %d", c, refused, any_bytes);
    if (in_only_overlap) CHECK(!refused, "canvas %d: inputs overlapping inputs were refused", c);
    if (refused && refuse) CHECK(bad.count({j.a, j.b}) == 1, "canvas %d: the pair %zu, %zu named is not an offending one", c, j.a, j.b);
}

// ---- boundaries ------------------------------------------------------------------------------------------------------------------
MViewsVerdict plan_of(const std::vector<hgi_mview_pair> &v, uint32_t E, hgi_mviews_info *info = nullptr)
{
    std::vector<uint8_t> blob((size_t)views_blob_bytes(v.size()));
    hgi_mviews_info mine;
    return mviews_plan(v.data(), v.size(), E, blob.data(), info ? info : &mine).verdict;
}

void boundaries()
{
    // the page rule of the grid side: the last grid byte at every offset of its page
    for (uint32_t m = 1; m <= 3; ++m)
        for (uint32_t off = 0; off < 4096; ++off) {
            const uint32_t E = off & 1 ? 4 : 2;
            const uint32_t w = 4 * (1 + off % 3) + m, h = 1 + off % 4;
            const uint64_t sp = w + kGaps[off % 6], span = (uint64_t)(h - 1) * sp + w;
            const uint64_t src = (7ull << 32) + 4096 * 4 + off + 1 - span;
            const std::vector<hgi_mview_pair> v = {{1ull << 50, 2ull << 50, 8, 8, 8, 8 * E}, {src, 1ull << 52, w, h, sp, ((uint64_t)w + 3) * E}};
            const MViewsVerdict got = plan_of(v, E);
            CHECK(got == (off + 3 <= 4095 ? kMViewsOk : kMViewsTail), "page rule: width %% 4 = %u, last byte at %u: verdict %d", m, off, (int)got);
        }
    CHECK(plan_of({{(7ull << 32) + 4096 - 12 * 3, 1ull << 52, 12, 3, 12, 48}}, 4) == kMViewsOk, "page rule on dword rows");
    for (uint32_t E : {2u, 4u}) {
        // side_fits32 at its bound, on each side: the written side's pitch is in BYTES
        for (uint32_t h : {2u, 64u, 700u, 5000u}) {
            const uint64_t P = ((1ull << 32) - 1025) / ((uint64_t)h + 192) / 4 * 4;      // a multiple of E below the bound ...
            const uint64_t Q = P + 4;                                                    // ... and the next one is beyond it
            CHECK(side_fits32(h, P) && !side_fits32(h, Q), "bound of height %u", h);
            for (int side = 0; side < 2; ++side)
                for (int over = 0; over < 2; ++over) {
                    hgi_mview_pair e = {1ull << 50, 2ull << 50, 8, h, 8, 8 * E};
                    (side ? e.dst_pitch : e.src_pitch) = over ? Q : P;
                    CHECK(plan_of({e}, E) == (over ? kMViewsFits32 : kMViewsOk), "32-bit bound: E %u height %u side %d over %d", E, h, side, over);
                }
            // a width whose ELEMENTS fit and whose bytes do not: the byte pitch decides
            hgi_mview_pair wide = {1ull << 50, 2ull << 50, (uint32_t)(Q / E), h, Q / E, Q};
            CHECK(side_fits32(h, Q / E) && plan_of({wide}, E) == kMViewsFits32, "E %u height %u: the byte pitch of the written side decides", E, h);
        }
        // the element rules at their bounds
        hgi_mview_pair ok = {1ull << 50, 2ull << 50, 30, 8, 40, 30 * E};
        CHECK(plan_of({ok}, E) == kMViewsOk, "E %u: dst_pitch == width * E", E);
        hgi_mview_pair bad = ok;
        bad.dst_pitch = 30 * E - E;
        CHECK(plan_of({bad}, E) == kMViewsDstPitch, "E %u: dst_pitch one element short", E);
        bad = ok;
        bad.dst_pitch = 40 * E + E / 2;
        CHECK(plan_of({bad}, E) == kMViewsDstPitchAlign, "E %u: dst_pitch half an element off", E);
        bad.dst_pitch = 40 * E + 1;
        CHECK(plan_of({bad}, E) == kMViewsDstPitchAlign, "E %u: dst_pitch one byte off", E);
        bad = ok;
        bad.dst += E / 2;
        CHECK(plan_of({bad}, E) == kMViewsDstAlign, "E %u: dst half an element off", E);
        bad.dst = ok.dst + E;
        CHECK(plan_of({bad}, E) == kMViewsOk, "E %u: dst one element on", E);
        // a one-row frame never steps by its pitch: neither rule of the pitch is asked
        CHECK(plan_of({{1ull << 50, 2ull << 50, 8, 1, 1ull << 40, (1ull << 63) + 1}}, E) == kMViewsOk, "E %u: one row", E);
        // rule order: the HGI_EINVAL rules first, in the header's order
        bad = ok;
        bad.src = 0;
        bad.src_pitch = 29;
        CHECK(plan_of({ok, bad}, E) == kMViewsNullEntry, "NULL before pitch");
        bad = ok;
        bad.src_pitch = 29;
        bad.dst += 1;
        CHECK(plan_of({bad}, E) == kMViewsSrcPitch, "source pitch before the element rules");
        bad = ok;
        bad.dst += 1;
        bad.dst_pitch = 1;
        CHECK(plan_of({bad}, E) == kMViewsDstAlign, "dst before dst_pitch");
        bad = ok;
        bad.dst_pitch = 29 * E + 1;
        CHECK(plan_of({bad}, E) == kMViewsDstPitchAlign, "the multiple before the size");
        bad = ok;
        bad.dst = bad.src;      // in place, and a side beyond 32 bits
        bad.dst_pitch = bad.src_pitch = 1ull << 33;
        CHECK(plan_of({bad}, E) == kMViewsOutIn, "aliasing before the 32-bit rule");
        // an output's rectangle is width * E bytes wide: a neighbour E * width bytes on is fine, one element nearer is not
        hgi_mview_pair l = {1ull << 50, 2ull << 50, 30, 8, 40, 100 * E}, r = {3ull << 50, (2ull << 50) + 30 * E, 30, 8, 40, 100 * E};
        CHECK(plan_of({l, r}, E) == kMViewsOk, "E %u: side by side", E);
        r.dst -= E;
        CHECK(plan_of({l, r}, E) == kMViewsOutOut, "E %u: the last element shared", E);
        // ... and a grid that starts behind the width * E bytes of an output row, inside its pitch, is fine
        hgi_mview_pair g = {(2ull << 50) + 30 * E, 5ull << 50, 5, 8, 100 * E, 5 * E};
        CHECK(plan_of({l, g}, E) == kMViewsOk, "E %u: a grid in the output's gap", E);
        g.src -= 1;
        CHECK(plan_of({l, g}, E) == kMViewsOutIn, "E %u: a grid on the output's last byte", E);
        // rows of 2^32 bytes and more are judged as they are (aliasing, an HGI_EINVAL rule, before the 32-bit rule)
        const uint32_t W = 1u << 31;
        hgi_mview_pair big = {1ull << 50, 2ull << 50, W, 1, 0, 0}, tiny = {3ull << 50, (2ull << 50) + (uint64_t)W * E - E, 1, 1, 0, 0};
        CHECK(plan_of({big, tiny}, E) == kMViewsOutOut, "E %u: the last element of a row of 2^%d bytes", E, E == 2 ? 32 : 33);
        tiny.dst += E;
        CHECK(plan_of({big, tiny}, E) == kMViewsFits32, "E %u: the element behind it", E);
    }
    // the tile-count bound, in 64 bits
    {
        const uint32_t W = 128u << 16, H = 64u * 32767u;
        std::vector<hgi_mview_pair> v = {{1ull << 50, 1ull << 56, W, H, W, 2ull * W}, {1ull << 58, 1ull << 59, 128u * (65536u - 16u), 1, 0, 0}};
        CHECK(list_tiles(W, H) + list_tiles(v[1].width, 1) == (1ull << 31) - 16, "tiles of the boundary list");
        CHECK(plan_of(v, 2) == kMViewsFits32, "2^31 - 16 tiles pass the tile rule");
        v.push_back({1ull << 60, 1ull << 61, 1, 1, 1, 2});
        hgi_mviews_info info;
        memset(&info, 0x5A, sizeof(info));
        CHECK(plan_of(v, 2, &info) == kMViewsTiles && info.magic == 0x5A5A5A5Au, "2^31 - 15 tiles");
        const std::vector<hgi_mview_pair> many(3000, hgi_mview_pair{1ull << 50, 1ull << 56, 0xFFFFFFFFu, 0xFFFFFFFFu, 1ull << 32, 1ull << 34});
        CHECK(plan_of(many, 4) == kMViewsTiles, "3000 frames of 2^51 tiles");
    }
    {   // the plans of no frame, and what the launch notices of a changed info
        hgi_mview_pair empty = {0, 0, 0, 9, 0, 0};
        hgi_mviews_info info;
        CHECK(plan_of({empty, empty}, 2, &info) == kMViewsOk && info.count == 0 && info.magic == HGI_MVIEWS_MAGIC && mviews_info_consistent(info), "only empty entries");
        CHECK(plan_of({}, 4, &info) == kMViewsOk && info.count == 0 && info.dst_lo == 0 && info.dst_hi == 0 && mviews_info_consistent(info), "no entry");
        CHECK(plan_of({{1ull << 50, 2ull << 50, 30, 8, 40, 160}}, 4, &info) == kMViewsOk && mviews_info_consistent(info), "one entry");
        CHECK(info.dst_lo == 2ull << 50 && info.dst_hi == (2ull << 50) + 7 * 160 + 120, "its interval");
        hgi_mviews_info d = info;
        d.plan_bytes += 16;
        CHECK(!mviews_info_consistent(d), "a changed size is noticed");
        d = info;
        d.elem_size = 3;
        CHECK(!mviews_info_consistent(d), "a changed element size is noticed");
        d = info;
        d.magic = HGI_VIEWS_MAGIC;
        CHECK(!mviews_info_consistent(d), "the view lists' magic is not this library's");
        d = info;
        d.dst_hi = d.dst_lo;
        CHECK(!mviews_info_consistent(d), "an empty output interval is noticed");
    }
}

}  // namespace

int main(int argc, char **argv)
{
    const int cases = argc > 1 ? atoi(argv[1]) : 2000;
    if (argc > 2) g_x = strtoull(argv[2], nullptr, 0) | 1u;
    for (int c = 0; c < cases; ++c) {
        one_list(c);
        one_canvas(c);
    }
    boundaries();
    std::printf("mviews plan: %d cases, %d failures\n", cases, g_bad);
    return g_bad ? 1 : 0;
}
