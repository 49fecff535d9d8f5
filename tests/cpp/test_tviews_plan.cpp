// rustyhgi_amd/tviews/hgi_tviews_plan.h -- the host plan of the typed view lists -- under ASan / UBSan, a stand-alone program:
//   * per-frame geometry: on random small lists (1 ... 40 entries, sides 0 ... 700, E in {2, 4}, frame pitches (w + gap) * E bytes,
//     grid pitches w + gap bytes) the record and the prefix sums against typed_plan of a batch of one, field by field -- the
//     written side and the tile counts its pitched plan's, the read side in BYTES: sp32 the byte pitch, srec the span
//     (h - 1) * pitch + w * E, plus 2 where E = 2 and the width is odd; every tile origin of both sides formed in 32 bits as the
//     kernel forms it equals the one formed in 64; every block of the launch walked through view_block (the view lists' map, run
//     unchanged): every tile of every non-empty frame exactly once;
//   * aliasing: on random canvases of up to 192 x 48 bytes against a brute-force byte-set model with w * E bytes wide input
//     rectangles -- same-pitch placements agree exactly, both ways, one-row views against any pitch; span-meeting views of more
//     than one row and different pitches are refused; frames overlapping frames are accepted;
//   * boundary rules, both sides of each boundary: the per-entry page rule at end % 4096 in {0, 2, 4094} and at every even
//     residue; no page rule on the grid side, at E = 4 or at even widths; side_fits32 at its bound on each side, the read
//     side's in bytes; the element rules (src and src_pitch multiples of E, src_pitch >= w * E, dst_pitch >= w) at their bounds;
//     the tile-count bound; the order of the rules; rows of 2^32 bytes and more.
// Nothing here touches frame memory.  Usage: test_tviews_plan [lists] [seed]
#include <cstring>
#include <set>

#include "../../rustyhgi_amd/tviews/hgi_tviews_plan.h"
#include "plan_test_util.h"

using namespace hgi;

namespace {

const uint32_t kGaps[6] = {0, 1, 3, 16, 61, 128};

bool page_rule(const hgi_tview_pair &v, uint32_t E)      // include/hgi_tviews.h, restated
{
    if (E != 2 || v.width % 2 == 0) return true;
    const uint64_t end = v.src + (uint64_t)(v.height - 1) * (v.height > 1 ? v.src_pitch : 2ull * v.width) + 2ull * v.width;
    return end % 4096 != 0;
}

void one_list(int c)
{
    const uint32_t E = rnd_in(0, 1) ? 4 : 2;
    const size_t n = c % 16 == 15 ? 1 : (size_t)rnd_in(1, 40);
    std::vector<hgi_tview_pair> v(n);
    uint64_t at = (1ull << 40) + rnd_in(0, 4095);
    for (size_t i = 0; i < n; ++i) {
        uint32_t w = (uint32_t)rnd_in(0, 700), h = (uint32_t)rnd_in(0, 700);
        if (c % 16 == 14) w = 128 * (uint32_t)rnd_in(1, 5), h = 64 * (uint32_t)rnd_in(1, 6);
        v[i].width = w;
        v[i].height = h;
        v[i].src_pitch = (uint64_t)(w + kGaps[rnd_in(0, 5)]) * E;
        v[i].dst_pitch = w + kGaps[rnd_in(0, 5)];
        v[i].src = (at + rnd_in(0, 130) + E - 1) / E * E;
        if (c % 8 == 3 && w && h && E == 2 && (w & 1)) {      // some odd-width frames end on a page boundary
            const uint64_t end = v[i].src + (uint64_t)(h - 1) * (h > 1 ? v[i].src_pitch : 2ull * w) + 2ull * w;
            v[i].src += (4096 - end % 4096) % 4096;
        }
        at = v[i].src + (uint64_t)h * v[i].src_pitch + 8 + rnd_in(0, 300);
        v[i].dst = at + rnd_in(0, 130);
        at = v[i].dst + (uint64_t)h * v[i].dst_pitch + 8 + rnd_in(0, 300);
    }
    std::vector<uint8_t> blob((size_t)views_blob_bytes(n) + 1, 0xAB);
    hgi_tviews_info info;
    memset(&info, 0x5A, sizeof(info));
    const TViewsJudged j = tviews_plan(v.data(), n, E, blob.data(), &info);
    size_t first_tail = n;
    for (size_t i = n; i-- > 0;)
        if (v[i].width && v[i].height && !page_rule(v[i], E)) first_tail = i;
    if (first_tail < n) {
        CHECK(j.verdict == kTViewsTail && j.a == first_tail, "list %d: page rule of view %zu, verdict %d at %zu", c, first_tail, (int)j.verdict, j.a);
        CHECK(info.magic == 0x5A5A5A5Au && blob[0] == 0xAB, "list %d: a refused plan wrote something", c);
        return;
    }
    CHECK(j.verdict == kTViewsOk, "list %d: verdict %d at %zu", c, (int)j.verdict, j.a);
    if (j.verdict != kTViewsOk) return;
    CHECK(blob.back() == 0xAB && tviews_info_consistent(info) && info.elem_size == E, "list %d: blob size / info", c);
    const ViewArgs a = tview_args(blob.data(), info);
    std::vector<size_t> idx;
    for (size_t i = 0; i < n; ++i)
        if (v[i].width && v[i].height) idx.push_back(i);
    const uint32_t m = info.count;
    CHECK(m == idx.size(), "list %d: %u records, %zu non-empty views", c, m, idx.size());
    if (m != idx.size()) return;
    uint64_t ne = 0, ni = 0;
    uint32_t wmax = 0;
    std::vector<std::vector<uint8_t>> seen(m);
    for (uint32_t f = 0; f < m; ++f) {
        const hgi_tview_pair &s = v[idx[f]];
        // typed_plan of a batch of one: the grid's pitched plan and the frame's side in bytes
        const TypedFrames tf = {s.width, s.height, 1u, E, s.src_pitch, s.dst_pitch, 0, 0};
        const TypedJudged t = typed_plan(s.src, tf);
        const PitchedPlan &p = t.plan.p;
        const uint64_t ip = s.height > 1 ? s.src_pitch : (uint64_t)s.width * E;
        const uint64_t ispan = (uint64_t)(s.height - 1) * ip + (uint64_t)s.width * E + (E == 2 && (s.width & 1) ? 2 : 0);
        const uint64_t gp = s.height > 1 ? s.dst_pitch : s.width, gspan = (uint64_t)(s.height - 1) * gp + s.width;
        ViewFrame F;
        memcpy(&F, a.frames + f, sizeof(F));
        CHECK(p.fast == 1 && p.ok && t.fits32 && t.tail_ok, "list %d view %zu: an accepted view is not on the buffer path", c, idx[f]);
        CHECK(F.src == s.src && F.dst == s.dst && F.width == p.W && F.height == p.H && F.width == s.width && F.height == s.height, "list %d frame %u: record", c, f);
        CHECK(F.full_x == p.ix && F.full_y == p.iy && view_tiles_x(F.width) == p.tx && view_tiles_y(F.height) == p.ty, "list %d frame %u: tiles", c, f);
        CHECK(F.sp32 == t.plan.x.pitch32 && F.srec == t.plan.x.rec && F.sp32 == ip && F.srec == ispan, "list %d frame %u: read side %u / %u, want %llu / %llu", c, f, F.sp32,
              F.srec, (unsigned long long)ip, (unsigned long long)ispan);
        CHECK(F.dp32 == p.dp32 && F.drec == p.drec && F.dp32 == gp && F.drec == gspan, "list %d frame %u: written side", c, f);
        CHECK(memcmp(&F.fd_fx, &p.fd_ix, sizeof(FastDiv)) == 0, "list %d frame %u: divisor", c, f);
        CHECK(a.epre[f] == ne && a.ipre[f] == ni, "list %d frame %u: prefix", c, f);
        ne += p.epf;
        ni += p.ipf;
        wmax = s.width > wmax ? s.width : wmax;
        seen[f].assign((size_t)p.tx * p.ty, 0);
    }
    CHECK(info.edge_tiles == ne && info.interior_tiles == ni && info.max_width == wmax, "list %d: totals", c);
    // every block, through the view lists' map; both sides' tile origins in 32 bits
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
        const uint32_t X0 = r.tx * 128, Y0 = r.ty * 64, rb = Y0 * F.sp32 + X0 * E, wb = Y0 * F.dp32 + X0;
        CHECK(rb == (uint64_t)Y0 * F.sp32 + (uint64_t)X0 * E && wb == (uint64_t)Y0 * F.dp32 + X0, "list %d block %llu: a tile origin wraps", c, (unsigned long long)b);
        // the largest offset the typed staging forms on the read side (companion/hgi_sides.h) stays in 32 bits
        CHECK((uint64_t)(Y0 + 128) * F.sp32 + (uint64_t)(X0 + 208) * E < (1ull << 32), "list %d block %llu: read side beyond 32 bits", c, (unsigned long long)b);
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
    std::vector<hgi_tview_pair> v(n);
    std::vector<Side> sides;
    for (size_t i = 0; i < n; ++i) {
        const uint32_t we = CP / E;      // the canvas' width in elements
        const uint32_t w = (uint32_t)rnd_in(1, we > 12 ? we / 3 : we), h = (uint32_t)rnd_in(1, CH > 9 ? CH / 3 : CH);
        uint64_t pitch[2], p[2];
        for (int o = 0; o < 2; ++o) {
            const uint32_t e = o ? 1 : E;      // side 0 is the frame, placed on whole elements; side 1 the grid
            if (mixed && rnd_in(0, 1)) {       // a pitch of its own, anywhere in the canvas' bytes
                pitch[o] = (uint64_t)(w + rnd_in(0, 9)) * e;
                const uint64_t span = (uint64_t)(h - 1) * pitch[o] + (uint64_t)w * e;
                p[o] = base + (span < bytes ? rnd_in(0, (bytes - span) / e) * e : 0);
            } else {                           // a window of the canvas
                pitch[o] = CP;
                p[o] = base + rnd_in(0, CH - h) * CP + rnd_in(0, (CP - w * e) / e) * e;
            }
        }
        if (in_only_overlap) {                 // grids far away and apart: only frames can meet
            pitch[1] = w;
            p[1] = (1ull << 40) + i * 65536;
        }
        v[i] = hgi_tview_pair{p[0], p[1], w, h, pitch[0], pitch[1]};
        sides.push_back(Side{p[0], pitch[0], (uint64_t)w * E, h, i, false});
        sides.push_back(Side{p[1], pitch[1], w, h, i, true});
    }
    // the model: a pair with a grid in it is refused iff its spans meet and (the pitches differ or the byte sets meet)
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
    hgi_tviews_info info;
    const TViewsJudged j = tviews_plan(v.data(), n, E, blob.data(), &info);
    const bool refused = j.verdict == kTViewsOutOut || j.verdict == kTViewsOutIn;
    CHECK(refused || j.verdict == kTViewsOk || j.verdict == kTViewsTail, "canvas %d: verdict %d", c, (int)j.verdict);
    CHECK(refused == refuse, "canvas %d (%zu views, E %u, mixed %d): refused %d, model %d", c, n, E, mixed, refused, refuse);
    if (all_same) CHECK(refused == any_bytes, "canvas %d: same pitches, refused %d, bytes shared %d", c, refused, any_bytes);
    if (in_only_overlap) CHECK(!refused, "canvas %d: frames overlapping frames were refused", c);
    if (refused && refuse) CHECK(bad.count({j.a, j.b}) == 1, "canvas %d: the pair %zu, %zu named is not an offending one", c, j.a, j.b);
}

// ---- boundaries ------------------------------------------------------------------------------------------------------------------
TViewsVerdict plan_of(const std::vector<hgi_tview_pair> &v, uint32_t E, hgi_tviews_info *info = nullptr)
{
    std::vector<uint8_t> blob((size_t)views_blob_bytes(v.size()));
    hgi_tviews_info mine;
    return tviews_plan(v.data(), v.size(), E, blob.data(), info ? info : &mine).verdict;
}

void boundaries()
{
    // the page rule, per entry on its own span: E = 2 and an odd width, the span's end at every even residue of a page -- 0 is
    // refused, 2 and 4094 (and every other one) are served; the entry in front of it and the one behind it do not matter
    for (uint32_t res = 0; res < 4096; res += 2) {
        const uint32_t w = 2 * (1 + res % 7) + 1, h = 1 + (res / 2) % 4;
        const uint64_t sp = 2ull * (w + kGaps[(res / 2) % 6]), span = (uint64_t)(h - 1) * (h > 1 ? sp : 2ull * w) + 2ull * w;
        const uint64_t src = (7ull << 32) + 4096 * 4 + res - span;
        const std::vector<hgi_tview_pair> v = {{1ull << 50, 2ull << 50, 8, 8, 16, 8}, {src, 1ull << 52, w, h, sp, (uint64_t)w + 3}, {3ull << 50, 6ull << 50, 8, 8, 16, 8}};
        CHECK((src + span) % 4096 == res, "page rule: the case's own arithmetic");
        const TViewsVerdict got = plan_of(v, 2);
        CHECK(got == (res == 0 ? kTViewsTail : kTViewsOk), "page rule: end %% 4096 = %u, width %u height %u: verdict %d", res, w, h, (int)got);
        if (res == 0 || res == 2 || res == 4094) {
            // an even width, or the same bytes as 4-byte elements (the span ends where it ended), is served at every end
            std::vector<hgi_tview_pair> e = v;
            e[1].width = w + 1;
            e[1].src = src - 2;
            e[1].src_pitch = sp + 2;
            e[1].dst_pitch = w + 4;
            CHECK(plan_of(e, 2) == kTViewsOk, "page rule: an even width at end %% 4096 = %u", res);
            // no page rule on the grid side: a grid whose span ends on a page boundary
            e = v;
            e[1].src = src + (res == 4094 ? 4 : 2);      // (the frame's end off the boundary)
            e[1].dst = (1ull << 52) + 4096 - ((uint64_t)(h - 1) * (h > 1 ? w + 3 : w) + w);
            CHECK(plan_of(e, 2) == kTViewsOk, "no page rule on the grid side");
        }
    }
    for (uint32_t w : {3u, 5u}) {      // E = 4: an odd width ending on a page boundary is served
        const hgi_tview_pair e = {(7ull << 32) + 4096 - (2ull * 4 * (w + 1) + 4ull * w), 1ull << 52, w, 3, 4ull * (w + 1), w};
        CHECK((e.src + 2 * e.src_pitch + 4ull * w) % 4096 == 0 && plan_of({e}, 4) == kTViewsOk, "E = 4 has no page rule");
    }
    for (uint32_t E : {2u, 4u}) {
        // side_fits32 at its bound, on each side: the read side's pitch is in BYTES
        for (uint32_t h : {2u, 64u, 700u, 5000u}) {
            const uint64_t P = ((1ull << 32) - 1025) / ((uint64_t)h + 192) / 4 * 4;      // a multiple of E below the bound ...
            const uint64_t Q = P + 4;                                                    // ... and the next one is beyond it
            CHECK(side_fits32(h, P) && !side_fits32(h, Q), "bound of height %u", h);
            for (int side = 0; side < 2; ++side)
                for (int over = 0; over < 2; ++over) {
                    hgi_tview_pair e = {1ull << 50, 2ull << 50, 8, h, 8 * E, 8};
                    (side ? e.dst_pitch : e.src_pitch) = over ? Q : P;
                    CHECK(plan_of({e}, E) == (over ? kTViewsFits32 : kTViewsOk), "32-bit bound: E %u height %u side %d over %d", E, h, side, over);
                }
            // a width whose ELEMENTS fit and whose bytes do not: the byte pitch decides
            hgi_tview_pair wide = {1ull << 50, 2ull << 50, (uint32_t)(Q / E), h, Q, Q / E};
            CHECK(side_fits32(h, Q / E) && plan_of({wide}, E) == kTViewsFits32, "E %u height %u: the byte pitch of the read side decides", E, h);
        }
        // the element rules at their bounds
        hgi_tview_pair ok = {1ull << 50, 2ull << 50, 30, 8, 30 * E, 30};
        CHECK(plan_of({ok}, E) == kTViewsOk, "E %u: src_pitch == width * E, dst_pitch == width", E);
        hgi_tview_pair bad = ok;
        bad.src_pitch = 30 * E - E;
        CHECK(plan_of({bad}, E) == kTViewsSrcPitch, "E %u: src_pitch one element short", E);
        bad = ok;
        bad.src_pitch = 40 * E + E / 2;
        CHECK(plan_of({bad}, E) == kTViewsSrcPitchAlign, "E %u: src_pitch half an element off", E);
        bad.src_pitch = 40 * E + 1;
        CHECK(plan_of({bad}, E) == kTViewsSrcPitchAlign, "E %u: src_pitch one byte off", E);
        bad = ok;
        bad.src += E / 2;
        CHECK(plan_of({bad}, E) == kTViewsSrcAlign, "E %u: src half an element off", E);
        bad.src = ok.src + E;
        CHECK(plan_of({bad}, E) == kTViewsOk, "E %u: src one element on", E);
        bad = ok;
        bad.dst_pitch = 29;
        CHECK(plan_of({bad}, E) == kTViewsDstPitch, "E %u: dst_pitch one byte short", E);
        bad = ok;
        bad.dst += 1;
        CHECK(plan_of({bad}, E) == kTViewsOk, "E %u: the grid lies at any byte", E);
        // a one-row frame never steps by its pitch: no rule of a pitch is asked
        CHECK(plan_of({{1ull << 50, 2ull << 50, 8, 1, (1ull << 63) + 1, 1ull << 40}}, E) == kTViewsOk, "E %u: one row", E);
        // rule order: the HGI_EINVAL rules first, in the header's order
        bad = ok;
        bad.dst = 0;
        bad.src += 1;
        CHECK(plan_of({ok, bad}, E) == kTViewsNullEntry, "NULL before the alignment");
        bad = ok;
        bad.src += 1;
        bad.src_pitch = 40 * E + 1;
        CHECK(plan_of({bad}, E) == kTViewsSrcAlign, "src before src_pitch");
        bad = ok;
        bad.src_pitch = 29 * E + 1;
        CHECK(plan_of({bad}, E) == kTViewsSrcPitchAlign, "the multiple before the size");
        bad = ok;
        bad.src_pitch = 29 * E;
        bad.dst_pitch = 29;
        CHECK(plan_of({bad}, E) == kTViewsSrcPitch, "the source pitch before the grid's");
        bad = ok;
        bad.dst = bad.src;      // in place, and a side beyond 32 bits
        bad.dst_pitch = bad.src_pitch = 1ull << 33;
        CHECK(plan_of({bad}, E) == kTViewsOutIn, "aliasing before the 32-bit rule");
        // a frame's rectangle is width * E bytes wide: a grid that starts behind the width * E bytes of a frame row, inside its
        // pitch, is fine; one byte nearer is not
        hgi_tview_pair l = {1ull << 50, 2ull << 50, 30, 8, 100 * E, 40};
        hgi_tview_pair g = {5ull << 50, (1ull << 50) + 30 * E, 5, 8, 5 * E, 100 * E};
        CHECK(plan_of({l, g}, E) == kTViewsOk, "E %u: a grid in the frame's gap", E);
        g.dst -= 1;
        CHECK(plan_of({l, g}, E) == kTViewsOutIn, "E %u: a grid on the frame's last byte", E);
        // grids side by side are fine, one byte nearer is not; frames may share everything
        hgi_tview_pair a = {1ull << 50, 2ull << 50, 30, 8, 30 * E, 100}, b = {1ull << 50, (2ull << 50) + 30, 30, 8, 30 * E, 100};
        CHECK(plan_of({a, b}, E) == kTViewsOk, "E %u: grids side by side, one frame read twice", E);
        b.dst -= 1;
        CHECK(plan_of({a, b}, E) == kTViewsOutOut, "E %u: the last grid byte shared", E);
        // rows of 2^32 bytes and more are judged as they are (aliasing, an HGI_EINVAL rule, before the 32-bit rule)
        const uint32_t W = 1u << 31;
        hgi_tview_pair big = {1ull << 50, 2ull << 50, W, 1, 0, 0}, tiny = {3ull << 50, (1ull << 50) + (uint64_t)W * E - 1, 1, 1, 0, 0};
        CHECK(plan_of({big, tiny}, E) == kTViewsOutIn, "E %u: the last byte of a frame row of 2^%d bytes", E, E == 2 ? 32 : 33);
        tiny.dst += 1;
        CHECK(plan_of({big, tiny}, E) == kTViewsFits32, "E %u: the byte behind it", E);
    }
    // the tile-count bound, in 64 bits
    {
        const uint32_t W = 128u << 16, H = 64u * 32767u;
        std::vector<hgi_tview_pair> v = {{1ull << 50, 1ull << 56, W, H, 2ull * W, W}, {1ull << 58, 1ull << 59, 128u * (65536u - 16u), 1, 0, 0}};
        CHECK(list_tiles(W, H) + list_tiles(v[1].width, 1) == (1ull << 31) - 16, "tiles of the boundary list");
        CHECK(plan_of(v, 2) == kTViewsFits32, "2^31 - 16 tiles pass the tile rule");
        v.push_back({1ull << 60, 1ull << 61, 1, 1, 2, 1});
        hgi_tviews_info info;
        memset(&info, 0x5A, sizeof(info));
        CHECK(plan_of(v, 2, &info) == kTViewsTiles && info.magic == 0x5A5A5A5Au, "2^31 - 15 tiles");
        const std::vector<hgi_tview_pair> many(3000, hgi_tview_pair{1ull << 50, 1ull << 56, 0xFFFFFFFFu, 0xFFFFFFFFu, 1ull << 34, 1ull << 32});
        CHECK(plan_of(many, 4) == kTViewsTiles, "3000 frames of 2^51 tiles");
    }
    {   // the plans of no frame, and what the launch notices of a changed info
        hgi_tview_pair empty = {0, 0, 0, 9, 0, 0};
        hgi_tviews_info info;
        CHECK(plan_of({empty, empty}, 2, &info) == kTViewsOk && info.count == 0 && info.magic == HGI_TVIEWS_MAGIC && tviews_info_consistent(info), "only empty entries");
        CHECK(plan_of({}, 4, &info) == kTViewsOk && info.count == 0 && tviews_info_consistent(info), "no entry");
        CHECK(plan_of({{1ull << 50, 2ull << 50, 30, 8, 160, 40}}, 4, &info) == kTViewsOk && tviews_info_consistent(info), "one entry");
        hgi_tviews_info d = info;
        d.plan_bytes += 16;
        CHECK(!tviews_info_consistent(d), "a changed size is noticed");
        d = info;
        d.elem_size = 3;
        CHECK(!tviews_info_consistent(d), "a changed element size is noticed");
        d = info;
        d.magic = HGI_VIEWS_MAGIC;
        CHECK(!tviews_info_consistent(d), "the view lists' magic is not this library's");
        d = info;
        d.magic = HGI_MVIEWS_MAGIC;
        CHECK(!tviews_info_consistent(d), "the mapped view lists' magic is not this library's");
        static_assert(HGI_TVIEWS_MAGIC != HGI_VIEWS_MAGIC && HGI_TVIEWS_MAGIC != HGI_MVIEWS_MAGIC, "a magic of its own");
        static_assert(sizeof(hgi_tviews_info) == sizeof(hgi_views_info) && sizeof(hgi_tview_pair) == 40, "hgi_views_info's layout");
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
    std::printf("tviews plan: %d cases, %d failures\n", cases, g_bad);
    return g_bad ? 1 : 0;
}
