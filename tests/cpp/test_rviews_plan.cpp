// rustyhgi_amd/rviews/hgi_rviews_plan.h -- the host plan of the recon view lists and the judgement of their launch -- under
// ASan / UBSan, a stand-alone program:
//   * random lists (1 ... 24 frames, sides 0 ... 1500, pitches w + gap drawn per side, odd bases) laid out one behind the other
//     go through rviews_plan: the first views_blob_bytes(count) bytes of the blob are byte for byte what views_plan writes for
//     the (src, grid) pairs, the third-side records behind them are what extra_side / side_span give for a batch of one, the info
//     says so, and the launcher's block count follows from the info;
//   * windows in a small arena of bytes, three per entry, placed at random with one pitch or with two: the aliasing verdict
//     against marked bytes (inputs may overlap; all 2 * count outputs pairwise disjoint; no output meets an input), and the pair
//     the verdict names -- list index and side -- does meet;
//   * every aliasing kind by hand: grid against recon of the same entry and of another, grid against grid, recon against recon,
//     an output against an input, each with the index and side named; overlapping inputs served; grid and recon windows side by
//     side in one parent's rows served, the same windows at different pitches refused;
//   * every rule alone, and every pair one call can break together, with the earlier rule reported; the 32-bit bound over the
//     largest of THREE pitches (only the recon pitch over it); the page rule on the source only;
//   * rview_find, the kernels' cycle-free frame search, against list_find: every tile index of random prefix arrays with runs of
//     repeated entries (frames without tiles of a kind), counts 0 ... 70 and at powers of two and their neighbours up to 2^20,
//     arrays that are not sorted (both stay below count), and both prefix arrays of every served blob at every block;
//   * rviews_judge: every rule alone and in pairs, the split of the levels, the identity table, the empty plan first, and the
//     sibling magics -- views, mviews, tviews, sviews -- refused, as theirs refuse this one's.
// Nothing here touches image memory.  Usage: test_rviews_plan [lists] [seed]
#include <cstring>

#include "../../include/hgi_mviews.h"
#include "../../include/hgi_sviews.h"
#include "../../include/hgi_tviews.h"
#include "../../rustyhgi_amd/rviews/hgi_rviews_plan.h"
#include "plan_test_util.h"

using namespace hgi;

namespace {

const uint32_t kGaps[6] = {0, 1, 3, 16, 61, 128};
const void *const kPlan = reinterpret_cast<const void *>(uintptr_t(1) << 40);      // an address, never read

// include/hgi_rviews.h, restated: the page rule of an entry's own source span
bool tail_fits(const hgi_rview_triple &t)
{
    const uint64_t end = t.src + (uint64_t)(t.height - 1) * (t.height > 1 ? t.src_pitch : 0) + t.width;
    return t.width % 4 == 0 || ((end - 1) >> 12) == ((end + 2) >> 12);
}

struct Planned {
    RViewsJudged j;
    hgi_rviews_info info;
    std::vector<uint8_t> blob;      // one byte of 0xAB behind the most a plan of n entries may write
};

Planned plan_of(const std::vector<hgi_rview_triple> &v)
{
    Planned p;
    p.blob.assign((size_t)rviews_blob_bytes(v.size()) + 1, 0xAB);
    memset(&p.info, 0, sizeof(p.info));
    p.j = rviews_plan(v.data(), v.size(), p.blob.data(), &p.info);
    if (p.j.verdict != kRViewsOk) {
        bool clean = p.info.magic == 0;
        for (uint8_t b : p.blob) clean = clean && b == 0xAB;
        CHECK(clean, "a refused plan (%d) wrote something", (int)p.j.verdict);
    }
    return p;
}

void check_served(int c, const std::vector<hgi_rview_triple> &v, const Planned &p)
{
    const hgi_rviews_info &info = p.info;
    // the view lists' plan of the (src, grid) pairs
    std::vector<hgi_view_pair> pairs;
    for (const hgi_rview_triple &t : v) pairs.push_back(hgi_view_pair{t.src, t.grid, t.width, t.height, t.src_pitch, t.grid_pitch});
    std::vector<uint8_t> theirs((size_t)views_blob_bytes(v.size()) + 1, 0xAB);
    hgi_views_info vi;
    memset(&vi, 0, sizeof(vi));
    const ViewsJudged vj = views_plan(pairs.data(), pairs.size(), theirs.data(), &vi);
    CHECK(vj.verdict == kViewsOk, "case %d: the view lists refuse the (src, grid) pairs (%d)", c, (int)vj.verdict);
    if (vj.verdict != kViewsOk) return;
    CHECK(info.magic == HGI_RVIEWS_MAGIC && info.reserved == 0 && info.count == vi.count && info.edge_tiles == vi.edge_tiles &&
              info.interior_tiles == vi.interior_tiles && info.max_width == vi.max_width,
          "case %d: info against the view lists'", c);
    CHECK(info.records_offset == vi.records_offset && info.edge_prefix_offset == vi.edge_prefix_offset && info.interior_prefix_offset == vi.interior_prefix_offset &&
              info.recon_offset == vi.plan_bytes && info.recon_offset == views_blob_bytes(info.count) && info.plan_bytes == vi.plan_bytes + 16ull * info.count,
          "case %d: offsets", c);
    CHECK(rviews_info_consistent(info), "case %d: the plan's own info is inconsistent", c);
    CHECK(memcmp(p.blob.data(), theirs.data(), (size_t)vi.plan_bytes) == 0, "case %d: the blob's first %llu bytes are not views_plan's", c, (unsigned long long)vi.plan_bytes);
    CHECK(p.blob[(size_t)info.plan_bytes] == 0xAB, "case %d: the plan wrote behind plan_bytes", c);
    // the third sides
    uint64_t m = 0;
    for (size_t i = 0; i < v.size(); ++i) {
        const hgi_rview_triple &t = v[i];
        if (!t.width || !t.height) continue;
        RViewSide s;
        memcpy(&s, p.blob.data() + info.recon_offset + 16 * m, 16);
        const uint64_t rp = t.height > 1 ? t.recon_pitch : t.width;
        const ExtraSide x = extra_side(true, rp, side_span(t.width, t.height, rp), 0);
        CHECK(s.recon == t.recon && s.pitch32 == x.pitch32 && s.rec == x.rec, "case %d view %zu: third side %u %u", c, i, s.pitch32, s.rec);
        CHECK(s.pitch32 == rp && s.rec == (uint64_t)(t.height - 1) * rp + t.width, "case %d view %zu: third side in words", c, i);
        ViewFrame f;
        memcpy(&f, p.blob.data() + info.records_offset + 64 * m, 64);
        CHECK(f.src == t.src && f.dst == t.grid && f.width == t.width && f.height == t.height, "case %d view %zu: record", c, i);
        ++m;
    }
    CHECK(m == info.count, "case %d: count", c);
    // what the launch reads and the launcher's block count
    const RViewArgs a = rview_args(p.blob.data(), info);
    CHECK(reinterpret_cast<const uint8_t *>(a.recon) == p.blob.data() + info.recon_offset && a.v.count == info.count && a.v.nedge == info.edge_tiles &&
              a.v.nint == info.interior_tiles,
          "case %d: args", c);
    CHECK(rviews_blocks(info) == list_blocks(a.v.nedge, a.v.nint) && rviews_blocks(info) == ((info.edge_tiles + 7ull) & ~7ull) + info.interior_tiles,
          "case %d: block count", c);
    if (info.count) {
        // every block's frame has a third side: the walk stays inside the parallel array
        const uint64_t blocks = rviews_blocks(info);
        for (uint64_t b = 0; b < blocks; ++b) {
            const ListBlock r = view_block((uint32_t)b, a.v);
            if (r.idle) continue;
            CHECK(r.frame < info.count, "case %d: block %llu -> frame %u", c, (unsigned long long)b, r.frame);
            // ... and the kernels' search finds the frame the walk finds
            CHECK(rview_find(r.edge ? a.v.epre : a.v.ipre, a.v.count, r.t) == r.frame, "case %d: block %llu: rview_find differs from the walk", c, (unsigned long long)b);
        }
    }
}

void one_list(int c)
{
    const size_t n = c % 16 == 15 ? 1 : (size_t)rnd_in(1, 24);
    std::vector<hgi_rview_triple> v(n);
    uint64_t at = (1ull << 40) + rnd_in(0, 4095);
    for (size_t i = 0; i < n; ++i) {
        hgi_rview_triple &t = v[i];
        t.width = (uint32_t)rnd_in(0, 1500);
        t.height = (uint32_t)rnd_in(0, 1500);
        if (c % 4 == 1) t.width = 128 * (uint32_t)rnd_in(1, 4), t.height = 64 * (uint32_t)rnd_in(1, 4);
        t.src_pitch = t.width + kGaps[rnd_in(0, 5)];
        t.grid_pitch = t.width + kGaps[rnd_in(0, 5)];
        t.recon_pitch = t.width + kGaps[rnd_in(0, 5)];
        t.src = at + rnd_in(0, 130);
        while (t.width && t.height && !tail_fits(t)) ++t.src;
        at = t.src + (uint64_t)t.height * t.src_pitch + 8 + rnd_in(0, 300);
        t.grid = at + rnd_in(0, 130);
        at = t.grid + (uint64_t)t.height * t.grid_pitch + 8 + rnd_in(0, 300);
        t.recon = at + rnd_in(0, 130);
        at = t.recon + (uint64_t)t.height * t.recon_pitch + 8 + rnd_in(0, 300);
    }
    const Planned p = plan_of(v);
    CHECK(p.j.verdict == kRViewsOk, "case %d: a list of disjoint small frames refused (%d)", c, (int)p.j.verdict);
    if (p.j.verdict != kRViewsOk) return;
    check_served(c, v, p);
    // the launch's judgement on it
    uint8_t lut[256];
    const bool ident = rnd_in(0, 1) != 0;
    for (int i = 0; i < 256; ++i) lut[i] = (uint8_t)(ident ? i : 255 - i);
    const uint32_t levels = (uint32_t)rnd_in(1, 8);
    const RViewsLaunchJudged j = rviews_judge(kPlan, &p.info, levels, rnd_in(0, 1) ? HGI_INTERP_CROSSED : HGI_INTERP_LEFTTOP, lut);
    if (p.info.count == 0)
        CHECK(j.verdict == kRViewsEmpty && j.status == HGI_OK, "case %d: empty plan", c);
    else
        CHECK(j.verdict == kRViewsLaunch && j.status == HGI_OK && j.k == (levels < 6 ? levels : 4) && j.up == (levels < 6 ? 0 : levels - 4) && j.ident == ident && j.text[0] == 0,
              "case %d: served launch at %u levels", c, levels);
}

// ---- the frame search: rview_find against list_find ---------------------------------------------------------------------------
void check_find(const char *what, const std::vector<uint32_t> &pre, uint32_t count, uint32_t t)
{
    const uint32_t a = rview_find(pre.data(), count, t), b = list_find(pre.data(), count, t);
    CHECK(a == b && (count == 0 ? a == 0 : a < count), "%s: count %u t %u: rview_find %u, list_find %u", what, count, t, a, b);
}

void one_search(int c)
{
    uint32_t count = (uint32_t)rnd_in(0, 70);
    if (c % 8 == 7) count = (1u << rnd_in(1, 20)) + (uint32_t)rnd_in(0, 2) - 1;      // 2^k - 1, 2^k, 2^k + 1
    std::vector<uint32_t> pre(count + 1, 0);
    uint32_t total = 0;
    for (uint32_t i = 0; i < count; ++i) {
        pre[i] = total;
        total += rnd_in(0, 3) ? (uint32_t)rnd_in(1, 40) : 0;      // a frame in four has no tile of this kind: its successor's entry repeats
    }
    if (count <= 70)
        for (uint32_t t = 0; t <= total + 2; ++t) check_find("sorted", pre, count, t);
    else
        for (int k = 0; k < 200; ++k) check_find("sorted, large", pre, count, (uint32_t)rnd_in(0, (uint64_t)total + 2));
    check_find("t at the top", pre, count, 0xFFFFFFFFu);
    // a table that is not sorted: no equality is promised, both results stay inside the array
    for (uint32_t i = 0; i < count; ++i) pre[i] = (uint32_t)rnd();
    for (int k = 0; k < 8 && count; ++k) {
        const uint32_t t = (uint32_t)rnd();
        CHECK(rview_find(pre.data(), count, t) < count && list_find(pre.data(), count, t) < count, "search %d: a result outside an unsorted table", c);
    }
}

// ---- aliasing against marked bytes ---------------------------------------------------------------------------------------------
struct Rect {
    uint64_t lo;
    uint32_t w, h;
    uint64_t pitch;
    int side;      // 0 the input, 1 the grid, 2 the reconstruction
    size_t index;
};

bool bytes_meet(const Rect &a, const Rect &b, std::vector<uint8_t> &arena, uint64_t base)
{
    for (uint32_t y = 0; y < a.h; ++y) memset(&arena[(size_t)(a.lo - base + y * (a.h > 1 ? a.pitch : 0))], 1, a.w);
    bool hit = false;
    for (uint32_t y = 0; y < b.h && !hit; ++y)
        for (uint32_t x = 0; x < b.w && !hit; ++x) hit = arena[(size_t)(b.lo - base + y * (b.h > 1 ? b.pitch : 0) + x)] != 0;
    for (uint32_t y = 0; y < a.h; ++y) memset(&arena[(size_t)(a.lo - base + y * (a.h > 1 ? a.pitch : 0))], 0, a.w);
    return hit;
}

// 0: fine; 1: the bytes meet; 2: the spans meet at different pitches (refused without being judged)
int pair_meets(const Rect &a, const Rect &b, std::vector<uint8_t> &arena, uint64_t base)
{
    const uint64_t ahi = a.lo + (uint64_t)(a.h - 1) * (a.h > 1 ? a.pitch : 0) + a.w, bhi = b.lo + (uint64_t)(b.h - 1) * (b.h > 1 ? b.pitch : 0) + b.w;
    if (!(a.lo < bhi && b.lo < ahi)) return 0;
    if (a.h == 1 || b.h == 1 || a.pitch == b.pitch) return bytes_meet(a, b, arena, base) ? 1 : 0;
    return 2;
}

void one_arena(int c)
{
    const uint64_t base = 1ull << 41;
    const uint32_t P = (uint32_t)rnd_in(40, 96), P2 = c % 3 == 0 ? (uint32_t)rnd_in(40, 96) : P, rows = 48;
    const size_t n = (size_t)rnd_in(1, 4);
    std::vector<uint8_t> arena((size_t)rows * 96 * 6 + 4096, 0);
    std::vector<hgi_rview_triple> v(n);
    std::vector<Rect> rc;
    for (size_t i = 0; i < n; ++i) {
        hgi_rview_triple &t = v[i];
        const uint32_t w = 4 * (uint32_t)rnd_in(1, 9), h = (uint32_t)rnd_in(1, 20);      // (widths in dwords: no page rule in this arena)
        t.width = w;
        t.height = h;
        t.src_pitch = rnd_in(0, 3) ? P : P2;
        t.grid_pitch = rnd_in(0, 3) ? P : P2;
        t.recon_pitch = rnd_in(0, 3) ? P : P2;
        // images in the first third of the arena, grids mostly in the second, reconstructions mostly in the third: some lists are
        // served, some collide
        t.src = base + rnd_in(0, rows / 2) * t.src_pitch + rnd_in(0, t.src_pitch - w);
        t.grid = base + (rnd_in(0, 7) ? rows * 96 * (rnd_in(0, 7) ? 1 : 2) : 0) + rnd_in(0, rows / 2) * t.grid_pitch + rnd_in(0, t.grid_pitch - w);
        t.recon = base + (rnd_in(0, 7) ? rows * 96 * (rnd_in(0, 7) ? 2 : 1) : 0) + rnd_in(0, rows / 2) * t.recon_pitch + rnd_in(0, t.recon_pitch - w);
        rc.push_back(Rect{t.src, w, h, t.src_pitch, 0, i});
        rc.push_back(Rect{t.grid, w, h, t.grid_pitch, 1, i});
        rc.push_back(Rect{t.recon, w, h, t.recon_pitch, 2, i});
    }
    bool oo = false, oi = false;
    for (size_t x = 0; x < rc.size(); ++x)
        for (size_t y = x + 1; y < rc.size(); ++y) {
            const Rect &a = rc[x], &b = rc[y];
            if (!a.side && !b.side) continue;
            if (pair_meets(a, b, arena, base)) (a.side && b.side ? oo : oi) = true;
        }
    const Planned p = plan_of(v);
    const RViewsVerdict want = oo ? kRViewsOutOut : oi ? kRViewsOutIn : kRViewsOk;
    CHECK(p.j.verdict == want, "arena %d: verdict %d, bytes say %d", c, (int)p.j.verdict, (int)want);
    if (p.j.verdict == kRViewsOk) {
        check_served(c, v, p);
        return;
    }
    if (p.j.verdict != want) return;
    // the pair the verdict names, by index and side, does meet -- the way the verdict says
    const RViewsJudged &j = p.j;
    CHECK(j.a < n && j.b < n && (j.side_a == 0 || j.side_a == 1), "arena %d: the pair named", c);
    if (!(j.a < n && j.b < n)) return;
    const Rect &a = rc[3 * j.a + 1 + (size_t)j.side_a];
    const Rect &b = j.verdict == kRViewsOutOut ? rc[3 * j.b + 1 + (size_t)j.side_b] : rc[3 * j.b];
    if (j.verdict == kRViewsOutOut)
        CHECK(j.a < j.b || (j.a == j.b && j.side_a == kRViewsGrid && j.side_b == kRViewsRecon), "arena %d: two outputs in list order, the grid first", c);
    const int m = pair_meets(a, b, arena, base);
    CHECK(m != 0 && (m == 2) == j.mixed_pitch, "arena %d: the named pair (%zu side %d, %zu side %d) meets %d, mixed %d", c, j.a, j.side_a, j.b, j.side_b, m, (int)j.mixed_pitch);
}

// ---- every rule alone and in pairs -----------------------------------------------------------------------------------------------
const uint64_t A = 1ull << 42, B = 1ull << 43, C = 1ull << 44;
hgi_rview_triple good(int i)
{
    const uint64_t o = (uint64_t)i * (1ull << 30);
    return hgi_rview_triple{A + o, B + o, C + o, 300, 200, 320, 304, 384};
}

enum Rule { rNullEntry, rSrcPitch, rGridPitch, rReconPitch, rTiles, rOutOut, rOutIn, rFits32, rTail, rCount };
const RViewsVerdict kWant[rCount] = {kRViewsNullEntry, kRViewsSrcPitch, kRViewsGridPitch, kRViewsReconPitch, kRViewsTiles,
                                     kRViewsOutOut,    kRViewsOutIn,    kRViewsFits32,    kRViewsTail};

// breaks `r` in list `v` (entry 1 for the per-entry rules; rTiles is the giant entry that rules() puts into slot 2)
void breakit(std::vector<hgi_rview_triple> &v, Rule r)
{
    switch (r) {
    case rNullEntry: v[1].recon = 0; break;
    case rSrcPitch: v[1].src_pitch = v[1].width - 1; break;
    case rGridPitch: v[1].grid_pitch = 3; break;
    case rReconPitch: v[1].recon_pitch = v[1].width - 1; break;
    case rOutOut: v[3].recon = v[0].grid ? v[0].grid + 10 : 0, v[3].recon_pitch = v[0].grid_pitch; break;
    case rOutIn: v[4].grid = v[0].src + 5, v[4].grid_pitch = v[0].src_pitch; break;
    case rFits32: v[1].recon_pitch = 1ull << 32, v[1].recon = 1ull << 50; break;      // (far from every other span: aliasing is judged first)
    case rTail: v[1].width = 299, v[1].src = (A & ~4095ull) + (1ull << 30) + 3 * 4096 - (199 * 320 + 299); break;      // the span ends with its page
    default: break;
    }
}

void rules()
{
    for (int x = 0; x < rCount; ++x)
        for (int y = x; y < rCount; ++y) {
            std::vector<hgi_rview_triple> v;
            for (int i = 0; i < 5; ++i) v.push_back(good(i));
            v[2].width = 0;      // (the slot of the giant entry: empty unless rTiles)
            if (x == rReconPitch && y == rFits32) continue;      // one field, two values
            if (x == rTiles || y == rTiles) {
                // the giant entry: 2^49 tiles; it lies far from every other entry and is as legal as they are otherwise
                v[2] = hgi_rview_triple{1ull << 20, 0x5555555500000000ull, 0xAAAAAAAA00000000ull, 0xFFFFFFFFu, 0xFFFFFFFFu, 1ull << 32, 1ull << 32, 1ull << 32};
            }
            if (y != x) breakit(v, (Rule)y);      // (the later rule first: rTail changes the width the pitch rules are broken against)
            breakit(v, (Rule)x);
            const Planned p = plan_of(v);
            CHECK(p.j.verdict == kWant[x], "rules %d + %d: verdict %d, not the earlier rule's %d", x, y, (int)p.j.verdict, (int)kWant[x]);
            if (x <= rReconPitch || x >= rFits32) CHECK(p.j.a == 1, "rules %d + %d: names view %zu", x, y, p.j.a);
            if (x == rOutOut) CHECK(p.j.a == 0 && p.j.side_a == kRViewsGrid && p.j.b == 3 && p.j.side_b == kRViewsRecon, "rules %d + %d: names %zu/%d and %zu/%d", x, y, p.j.a, p.j.side_a, p.j.b, p.j.side_b);
            if (x == rOutIn) CHECK(p.j.a == 4 && p.j.side_a == kRViewsGrid && p.j.b == 0, "rules %d + %d: names views %zu and %zu", x, y, p.j.a, p.j.b);
        }
    // per entry the rules go in list order: an earlier entry's later rule is reported before a later entry's earlier rule
    {
        std::vector<hgi_rview_triple> v = {good(0), good(1)};
        v[0].recon_pitch = 3;
        v[1].src = 0;
        const Planned p = plan_of(v);
        CHECK(p.j.verdict == kRViewsReconPitch && p.j.a == 0, "list order");
    }
    // each NULL side of an entry
    for (int side = 0; side < 3; ++side) {
        std::vector<hgi_rview_triple> v = {good(0), good(1)};
        (side == 0 ? v[1].src : side == 1 ? v[1].grid : v[1].recon) = 0;
        const Planned p = plan_of(v);
        CHECK(p.j.verdict == kRViewsNullEntry && p.j.a == 1, "NULL side %d", side);
    }
    // what is not a fault: the pitches of a one-row frame, entries with a zero side whatever else they hold
    {
        std::vector<hgi_rview_triple> v = {good(0), good(1), good(2)};
        v[0].height = 1, v[0].src_pitch = 0, v[0].grid_pitch = 1, v[0].recon_pitch = 2;
        v[1] = hgi_rview_triple{0, 0, 0, 0, 9, 0, 0, 0};
        v[2].height = 0, v[2].src = 0;
        const Planned p = plan_of(v);
        CHECK(p.j.verdict == kRViewsOk && p.info.count == 1 && p.info.edge_tiles == 3 && p.info.interior_tiles == 0 && p.info.max_width == 300, "one-row frame, empty entries");
        RViewSide s;
        memcpy(&s, p.blob.data() + p.info.recon_offset, 16);
        CHECK(s.pitch32 == 300 && s.rec == 300 && s.recon == C, "a one-row frame's pitch counts as its width");
        check_served(-1, v, p);
    }
    // tiles are counted once per entry: the largest list of whole tiles the view lists serve is served here too
    {
        hgi_rview_triple e = good(0);
        e.width = 128 * 4096, e.height = 64 * 4094, e.src_pitch = e.grid_pitch = e.recon_pitch = e.width;      // 2^24 - 2^13 tiles
        e.src = 1ull << 40, e.grid = 1ull << 48, e.recon = 1ull << 56;
        std::vector<hgi_rview_triple> v(127, e);      // just under 2^31 tiles; inputs may overlap, the outputs may not
        for (size_t i = 0; i < v.size(); ++i) v[i].grid += i << 38, v[i].recon += i << 38;
        const Planned p = plan_of(v);
        CHECK(p.j.verdict == kRViewsFits32 || p.j.verdict == kRViewsOk, "a list below the tile bound is not refused for its tiles (%d)", (int)p.j.verdict);
        v.push_back(e);
        v.back().grid += 127ull << 38, v.back().recon += 127ull << 38;
        v.push_back(v.back());
        const Planned q = plan_of(v);
        hgi_view_pair vp = {e.src, e.grid, e.width, e.height, e.src_pitch, e.grid_pitch};
        std::vector<hgi_view_pair> pairs(v.size(), vp);
        std::vector<uint8_t> blob((size_t)views_blob_bytes(pairs.size()), 0);
        hgi_views_info vi;
        const bool theirs_tiles = views_plan(pairs.data(), pairs.size(), blob.data(), &vi).verdict == kViewsTiles;
        CHECK((q.j.verdict == kRViewsTiles) == theirs_tiles, "the tile bound is the view lists': once per entry (%d)", (int)q.j.verdict);
    }
}

// ---- the aliasing kinds, by hand ---------------------------------------------------------------------------------------------------
void aliasing()
{
    auto list = [] { return std::vector<hgi_rview_triple>{good(0), good(1), good(2)}; };
    struct Want {
        RViewsVerdict verdict;
        size_t a;
        int side_a;
        size_t b;
        int side_b;
    };
    auto expect = [](const char *what, const std::vector<hgi_rview_triple> &v, const Want &w, bool mixed = false) {
        const Planned p = plan_of(v);
        CHECK(p.j.verdict == w.verdict, "aliasing, %s: verdict %d", what, (int)p.j.verdict);
        if (p.j.verdict != w.verdict || w.verdict == kRViewsOk) return;
        CHECK(p.j.a == w.a && p.j.side_a == w.side_a && p.j.b == w.b && (w.verdict == kRViewsOutIn || p.j.side_b == w.side_b) && p.j.mixed_pitch == mixed,
              "aliasing, %s: names %zu/%d and %zu/%d, mixed %d", what, p.j.a, p.j.side_a, p.j.b, p.j.side_b, (int)p.j.mixed_pitch);
    };
    std::vector<hgi_rview_triple> v = list();
    v[1].recon = v[1].grid + 100 * 304 + 7, v[1].recon_pitch = 304;
    expect("grid against recon of the same entry", v, Want{kRViewsOutOut, 1, kRViewsGrid, 1, kRViewsRecon});
    v = list();
    v[2].recon = v[0].grid + 299, v[2].recon_pitch = 304;      // (its first byte is the last byte of the grid's first row)
    expect("grid against recon of another entry", v, Want{kRViewsOutOut, 0, kRViewsGrid, 2, kRViewsRecon});
    v = list();
    v[0].recon = v[2].grid + 199 * 304, v[0].recon_pitch = 304;
    expect("recon of an earlier entry against grid of a later one", v, Want{kRViewsOutOut, 0, kRViewsRecon, 2, kRViewsGrid});
    v = list();
    v[2].grid = v[1].grid + 1;
    expect("grid against grid", v, Want{kRViewsOutOut, 1, kRViewsGrid, 2, kRViewsGrid});
    v = list();
    v[1].recon = v[0].recon + 384 * 199 + 299;      // one byte: the last of entry 0's reconstruction
    expect("recon against recon", v, Want{kRViewsOutOut, 0, kRViewsRecon, 1, kRViewsRecon});
    v = list();
    v[1].grid = v[0].src + 64, v[1].grid_pitch = 320;
    expect("a grid against an input", v, Want{kRViewsOutIn, 1, kRViewsGrid, 0, 0});
    v = list();
    v[0].recon = v[2].src + 199 * 320 + 299, v[0].recon_pitch = 320;
    expect("a recon against an input", v, Want{kRViewsOutIn, 0, kRViewsRecon, 2, 0});
    v = list();
    v[1].recon = v[1].src;      // in place
    v[1].recon_pitch = v[1].src_pitch;
    expect("in place", v, Want{kRViewsOutIn, 1, kRViewsRecon, 1, 0});
    // overlapping inputs are served: two crops of one image, and one image twice
    v = list();
    v[1].src = v[0].src + 17 * 320 + 5, v[1].src_pitch = 320, v[2].src = v[0].src, v[2].src_pitch = 977;
    expect("overlapping inputs", v, Want{kRViewsOk, 0, 0, 0, 0});
    // grid and recon windows side by side in one parent's rows at one pitch: served, every entry, in either order
    v = list();
    for (int i = 0; i < 3; ++i) {
        v[i].grid_pitch = v[i].recon_pitch = 2048;
        v[i].grid = B + 600ull * i + (i == 1 ? 300 : 0);
        v[i].recon = B + 600ull * i + (i == 1 ? 0 : 300);
    }
    expect("windows side by side at one pitch", v, Want{kRViewsOk, 0, 0, 0, 0});
    check_served(-2, v, plan_of(v));
    // ... one byte nearer they share a column
    v[2].recon -= 1;
    expect("side by side, one byte nearer", v, Want{kRViewsOutOut, 2, kRViewsGrid, 2, kRViewsRecon});
    v[2].recon += 1;
    // ... and the same windows with different pitches are refused without being judged
    v[0].recon_pitch = 2049;
    expect("the same windows at different pitches", v, Want{kRViewsOutOut, 0, kRViewsGrid, 0, kRViewsRecon}, true);
    v = list();
    v[1].grid = v[0].src + 300, v[1].grid_pitch = 321;      // (it lies in the gap of the input's first row only)
    expect("an output and an input at different pitches", v, Want{kRViewsOutIn, 1, kRViewsGrid, 0, 0}, true);
    // the 32-bit bound is taken over the largest of three pitches: each pitch alone over it, the other two packed
    for (int side = 0; side < 3; ++side) {
        v = list();
        const uint64_t big = ((1ull << 32) - 1024) / (200 + 192) + 1;      // the smallest pitch that (height + 192) * P + 1024 puts at 2^32
        CHECK(!side_fits(200, big) && side_fits(200, big - 1), "the bound's edge");
        for (int d = 0; d < 2; ++d) {
            v[1].src_pitch = v[1].grid_pitch = v[1].recon_pitch = 300;
            (side == 0 ? v[1].src_pitch : side == 1 ? v[1].grid_pitch : v[1].recon_pitch) = big - d;
            v[1].src = 1ull << 50, v[1].grid = 1ull << 52, v[1].recon = 1ull << 54;
            const Planned p = plan_of(v);
            CHECK(p.j.verdict == (d ? kRViewsOk : kRViewsFits32) && (d || p.j.a == 1), "32-bit bound, side %d over by %d: %d", side, 1 - d, (int)p.j.verdict);
        }
    }
    // the page rule applies to the source only: outputs whose spans end with a page are served, the source's is not
    {
        const uint64_t span = 199ull * 320 + 299;
        v = list();
        for (auto &e : v) e.width = 299;
        v[1].grid_pitch = v[1].recon_pitch = 320;
        v[1].grid = B + (1ull << 30) + 20 * 4096 - span;
        v[1].recon = C + (1ull << 30) + 20 * 4096 - span;
        expect("outputs at the end of a page", v, Want{kRViewsOk, 0, 0, 0, 0});
        for (int back = 0; back < 5; ++back) {
            v[1].src = A + (1ull << 30) + 20 * 4096 - span - (uint64_t)back;
            const Planned p = plan_of(v);
            CHECK(p.j.verdict == (back < 3 ? kRViewsTail : kRViewsOk) && (back >= 3 || p.j.a == 1), "page rule, %d bytes in front of the page's end: %d", back, (int)p.j.verdict);
        }
        v[1].width = 300;      // a width in dwords reads nothing behind its span
        v[1].src = A + (1ull << 30) + 20 * 4096 - (199ull * 320 + 300);
        expect("a dword width at the end of a page", v, Want{kRViewsOk, 0, 0, 0, 0});
    }
}

// ---- the launch's judgement ------------------------------------------------------------------------------------------------------
hgi_rviews_info served_info()
{
    std::vector<hgi_rview_triple> v = {good(0), good(1)};
    const Planned p = plan_of(v);
    CHECK(p.j.verdict == kRViewsOk, "served_info");
    return p.info;
}

void judge()
{
    const void *odd = reinterpret_cast<const void *>((uintptr_t(1) << 40) + 8);
    uint8_t medium[256], identity[256];
    for (int i = 0; i < 256; ++i) medium[i] = (uint8_t)(i & ~3), identity[i] = (uint8_t)i;
    hgi_rviews_info ok = served_info(), broken = ok;
    broken.recon_offset += 16;
    struct Call {
        const void *d_plan;
        const hgi_rviews_info *info;
        uint32_t levels;
        int interp;      // (an int: an enumerator's value is not loaded from memory before the judgement has seen it)
        const uint8_t *lut;
    };
    const Call base = {kPlan, &ok, 6, 1, medium};
    CHECK(rviews_judge(base.d_plan, base.info, base.levels, (hgi_interp)base.interp, base.lut).verdict == kRViewsLaunch, "judge: the base call is served");
    // the rules in the header's order; each entry breaks one
    enum { jInfoNull, jInfo, jPlanNull, jPlanAlign, jLutNull, jLevelsRange, jInterp, jZero, jDepth, jCount };
    const RViewsLaunchVerdict want[jCount] = {kRViewsInfoNull, kRViewsInfo, kRViewsPlanNull, kRViewsPlanAlign, kRViewsLutNull, kRViewsLevelsRange, kRViewsInterp, kRViewsLevels, kRViewsLevels};
    auto apply = [&](Call &c, int r) {
        switch (r) {
        case jInfoNull: c.info = nullptr; break;
        case jInfo: c.info = &broken; break;
        case jPlanNull: c.d_plan = nullptr; break;
        case jPlanAlign: c.d_plan = odd; break;
        case jLutNull: c.lut = nullptr; break;
        case jLevelsRange: c.levels = 32; break;
        case jInterp: c.interp = 7; break;
        case jZero: c.levels = 0; break;
        case jDepth: c.levels = 9; break;
        }
    };
    for (int x = 0; x < jCount; ++x)
        for (int y = x; y < jCount; ++y) {
            if ((x == jInfoNull && y == jInfo) || (x == jPlanNull && y == jPlanAlign)) continue;                 // one argument, two values
            if (x >= jLevelsRange && y >= jLevelsRange && x != y && x != jInterp && y != jInterp) continue;      // `levels` has one value
            Call c = base;
            apply(c, y);
            apply(c, x);
            const RViewsLaunchJudged j = rviews_judge(c.d_plan, c.info, c.levels, (hgi_interp)c.interp, c.lut);
            CHECK(j.verdict == want[x] && j.status == (x < jZero ? HGI_EINVAL : HGI_EUNSUPPORTED) && j.text[0] != 0, "judge %d + %d: verdict %d status %d", x, y, (int)j.verdict, (int)j.status);
        }
    // every field of the info that the launch checks
    {
        auto refused = [&](const hgi_rviews_info &i, const char *what) {
            CHECK(rviews_judge(kPlan, &i, 4, HGI_INTERP_CROSSED, medium).verdict == kRViewsInfo, "judge: an info with a wrong %s accepted", what);
        };
        hgi_rviews_info i = ok;
        i.reserved = 1, refused(i, "reserved");
        i = ok, i.plan_bytes -= 16, refused(i, "plan_bytes");
        i = ok, i.plan_bytes = views_blob_bytes(i.count), refused(i, "plan_bytes (the view lists')");
        i = ok, i.records_offset = 64, refused(i, "records_offset");
        i = ok, i.edge_prefix_offset += 16, refused(i, "edge_prefix_offset");
        i = ok, i.interior_prefix_offset += 16, refused(i, "interior_prefix_offset");
        i = ok, i.recon_offset = 0, refused(i, "recon_offset");
        i = ok, i.recon_offset -= 16, refused(i, "recon_offset");
        i = ok, i.max_width = 0, refused(i, "max_width");
        i = ok, i.edge_tiles = 0, i.interior_tiles = 1, refused(i, "tile count");
        i = ok, i.interior_tiles = 0x7FFFFFF0u, refused(i, "block count");
        i = ok, i.count += 1, refused(i, "count");
    }
    // the split of the pyramid and the identity table, every depth
    for (uint32_t levels = 0; levels <= 40; ++levels)
        for (int id = 0; id < 2; ++id) {
            const RViewsLaunchJudged j = rviews_judge(kPlan, &ok, levels, HGI_INTERP_LEFTTOP, id ? identity : medium);
            if (levels > 31)
                CHECK(j.verdict == kRViewsLevelsRange && j.status == HGI_EINVAL, "judge: levels %u", levels);
            else if (levels == 0 || levels > 8)
                CHECK(j.verdict == kRViewsLevels && j.status == HGI_EUNSUPPORTED, "judge: levels %u", levels);
            else
                CHECK(j.verdict == kRViewsLaunch && j.status == HGI_OK && j.k == (levels <= 5 ? levels : 4) && j.up == (levels <= 5 ? 0 : levels - 4) && j.ident == (id != 0),
                      "judge: levels %u -> k %u up %u ident %d", levels, j.k, j.up, (int)j.ident);
        }
    {
        uint8_t nearly[256];
        memcpy(nearly, identity, 256);
        nearly[255] = 254;
        CHECK(!rviews_judge(kPlan, &ok, 4, HGI_INTERP_LEFTTOP, nearly).ident, "judge: a table that differs in its last entry is not the identity");
    }
    // the empty plan is decided first, whatever the other arguments
    {
        hgi_rviews_info e;
        memset(&e, 0, sizeof(e));
        CHECK(rviews_plan(nullptr, 0, nullptr, &e).verdict == kRViewsOk && e.magic == HGI_RVIEWS_MAGIC && e.count == 0 && e.plan_bytes == 0 && e.recon_offset == 0, "empty plan");
        for (uint32_t levels : {0u, 4u, 99u}) CHECK(rviews_judge(nullptr, &e, levels, (hgi_interp)-1, nullptr).verdict == kRViewsEmpty, "empty plan first");
        hgi_rview_triple z[2] = {{0, 0, 0, 0, 5, 0, 0, 0}, {0, 0, 0, 7, 0, 1, 1, 1}};
        uint8_t dummy[256];
        memset(&e, 0, sizeof(e));
        CHECK(rviews_plan(z, 2, dummy, &e).verdict == kRViewsOk && e.count == 0 && e.plan_bytes == 0 && rviews_blocks(e) == 0, "only empty entries");
        CHECK(rviews_judge(nullptr, &e, 4, (hgi_interp)9, nullptr).verdict == kRViewsEmpty, "only empty entries: nothing launched");
        hgi_rviews_info damaged = e;
        damaged.max_width = 1;
        CHECK(rviews_judge(kPlan, &damaged, 4, HGI_INTERP_CROSSED, medium).verdict == kRViewsInfo, "a damaged empty plan");
    }
    // the sibling magics are refused here ...
    for (uint32_t magic : {(uint32_t)HGI_VIEWS_MAGIC, (uint32_t)HGI_MVIEWS_MAGIC, (uint32_t)HGI_TVIEWS_MAGIC, (uint32_t)HGI_SVIEWS_MAGIC, 0u}) {
        hgi_rviews_info f = ok;
        f.magic = magic;
        CHECK(magic != HGI_RVIEWS_MAGIC && rviews_judge(kPlan, &f, 6, HGI_INTERP_CROSSED, medium).verdict == kRViewsInfo, "judge: magic %08x accepted", magic);
        f.count = f.edge_tiles = f.interior_tiles = f.max_width = 0;
        f.plan_bytes = f.edge_prefix_offset = f.interior_prefix_offset = f.recon_offset = 0;
        CHECK(rviews_judge(kPlan, &f, 6, HGI_INTERP_CROSSED, medium).verdict == kRViewsInfo, "judge: an empty plan of magic %08x accepted", magic);
    }
    // ... a real plan of the view lists too, and the view lists refuse this library's info
    {
        hgi_view_pair e = {A, B, 300, 200, 320, 320};
        std::vector<uint8_t> blob(512, 0);
        hgi_views_info theirs;
        CHECK(views_plan(&e, 1, blob.data(), &theirs).verdict == kViewsOk, "their plan");
        hgi_rviews_info mine;
        memset(&mine, 0, sizeof(mine));
        memcpy(&mine, &theirs, sizeof(theirs));
        mine.recon_offset = theirs.plan_bytes;
        CHECK(rviews_judge(kPlan, &mine, 6, HGI_INTERP_CROSSED, medium).verdict == kRViewsInfo, "judge: the view lists' plan accepted");
        static_assert(sizeof(hgi_rviews_info) == sizeof(hgi_views_info) + 8, "hgi_views_info's layout and one more field");
        memcpy(&theirs, &ok, sizeof(theirs));
        CHECK(!views_info_consistent(theirs), "the view lists accept this library's info");
        theirs.magic = HGI_VIEWS_MAGIC;
        CHECK(!views_info_consistent(theirs), "the view lists accept an info whose blob holds third sides");
    }
}

}  // namespace

int main(int argc, char **argv)
{
    const int cases = argc > 1 ? atoi(argv[1]) : 1500;
    if (argc > 2) g_x = strtoull(argv[2], nullptr, 0) | 1;
    rules();
    aliasing();
    judge();
    for (int c = 0; c < cases; ++c) {
        one_list(c);
        one_arena(c);
        one_search(c);
    }
    std::printf("%d cases, %d failures\n", cases, g_bad);
    return g_bad ? 1 : 0;
}
