// rustyhgi_amd/sviews/hgi_sviews_plan.h -- the host plan of the scaled view lists and the judgement of their launch -- under
// ASan / UBSan, a stand-alone program:
//   * random lists (1 ... 24 grids, sides 0 ... 1500, shifts 1 ... 6, pitches w + gap on each side, odd bases) laid out one behind
//     the other go through sviews_plan: every rule of include/hgi_sviews.h is restated here by brute force and must give the
//     plan's verdict; the record of a served grid holds the view -- sw x sh, src_pitch << s, the span, the output side;
//   * full_x / full_y against a per-byte model of what an interior tile's loads touch, at every depth a launch stages (one to
//     five levels in the tile): every view byte a tile needs lies in a dword that the descriptor's range check -- the grid's
//     span -- lets through, every row below the view reads behind the span (zeros), and no offset wraps 32 bits.  So an
//     interior tile reads nothing outside its grid's span and loses nothing inside it;
//   * the walk view_block covers every output tile of every grid exactly once, interior blocks inside full_x x full_y, ragged
//     ones outside, idle blocks only in the padding;
//   * windows in a small arena of bytes, placed at random with one pitch or with two: the aliasing verdict against marked bytes
//     (the input rectangle is the whole grid, the output rectangle sw x sh; inputs may overlap);
//   * every rule alone, and every pair one call can break together, with the earlier rule reported;
//   * sviews_judge: every rule alone and in pairs, the split of the remaining levels, the empty plan first, and foreign magics
//     both ways -- this judgement refuses the infos of the other view lists, and their consistency checks refuse this one's.
// Nothing here touches grid memory.  Usage: test_sviews_plan [lists] [seed]
#include <cstring>

#include "../../include/hgi_mviews.h"
#include "../../rustyhgi_amd/mviews/hgi_mviews_plan.h"
#include "../../rustyhgi_amd/sviews/hgi_sviews_plan.h"
#include "plan_test_util.h"

using namespace hgi;

namespace {

const uint32_t kGaps[6] = {0, 1, 3, 16, 61, 128};
const void *const kPlan = reinterpret_cast<const void *>(uintptr_t(1) << 40);      // an address, never read

uint32_t cdiv_pow2(uint32_t v, uint32_t s) { return (uint32_t)(((uint64_t)v + (1ull << s) - 1) >> s); }
int hoff_model(int idx) { return idx ? 2 << idx : 0; }      // hgi_fused_impl.h, hoff

struct Geo {      // include/hgi_sviews.h, restated
    uint32_t sw, sh;
    unsigned __int128 span, rp;
    uint64_t dp;
    bool read32, write32;
};

Geo geo(const hgi_sview_pair &v, uint32_t s)
{
    Geo g;
    g.sw = cdiv_pow2(v.width, s);
    g.sh = cdiv_pow2(v.height, s);
    g.span = (unsigned __int128)(v.height - 1) * (v.height > 1 ? v.src_pitch : 0) + v.width;
    g.rp = g.sh > 1 ? (unsigned __int128)v.src_pitch << s : g.span;
    const uint64_t tx = ((uint64_t)g.sw + 127) / 128, ty = ((uint64_t)g.sh + 63) / 64;
    g.read32 = g.span < ((unsigned __int128)1 << 32) && (unsigned __int128)(ty * 64 + 64) * g.rp + ((unsigned __int128)(tx * 128 + 80) << s) + 64 < ((unsigned __int128)1 << 32);
    g.dp = g.sh > 1 ? v.dst_pitch : g.sw;
    g.write32 = side_fits(g.sh, g.dp);
    return g;
}

// What an interior tile at (tx, ty) of a served grid's view reads, at nh halo rows: true when every byte it needs comes through
// the range check of a descriptor over `span` bytes and every row below the view reads zeros.
bool tile_loads_ok(const ViewFrame &f, uint32_t s, uint32_t tx, uint32_t ty, int nh, uint64_t *max_off)
{
    const uint64_t span = f.srec, rp = f.sp32;
    const uint64_t vb = (uint64_t)ty * 64 * rp + (((uint64_t)tx * 128) << s);
    bool ok = true;
    for (int r = 0; r < 64 + nh; ++r) {
        const int row = r < 64 ? r : 64 + hoff_model(r - 64);
        const uint64_t y = (uint64_t)ty * 64 + row;
        for (int c = 0; c < 8; ++c) {
            const uint64_t off = vb + (uint64_t)row * rp + ((16ull * c) << s);
            const uint64_t last = s <= 2 ? off + (16ull << s) - 1 : off + (15ull << s);
            if (last > *max_off) *max_off = last;
            if (y >= f.height) {      // below the view: every dword (byte) must be dropped
                ok = ok && off >= span;
                continue;
            }
            for (int j = 0; j < 16; ++j) {
                const uint64_t b = off + ((uint64_t)j << s);
                // s = 1, 2: wide loads, range-checked dword by dword (descriptor base = the grid's first byte); s >= 3: byte loads
                const uint64_t lo = s <= 2 ? off + ((b - off) & ~3ull) : b, hi = s <= 2 ? lo + 4 : b + 1;
                ok = ok && hi <= span;
                // ... and it is the byte of the lattice the view stands for
                ok = ok && b == y * rp + (((uint64_t)tx * 128 + 16 * c + j) << s);
            }
        }
    }
    return ok;
}

void check_served(int c, const std::vector<hgi_sview_pair> &v, uint32_t s, const std::vector<uint8_t> &blob, const hgi_sviews_info &info)
{
    uint64_t count = 0, ne = 0, ni = 0, wmax = 0;
    const ViewArgs a = sview_args(blob.data(), info);
    std::vector<std::vector<uint8_t>> seen;
    for (size_t i = 0; i < v.size(); ++i) {
        if (!v[i].width || !v[i].height) continue;
        const Geo g = geo(v[i], s);
        ViewFrame f;
        memcpy(&f, blob.data() + 64 * count, 64);
        uint32_t pe, pi;
        memcpy(&pe, blob.data() + info.edge_prefix_offset + 4 * count, 4);
        memcpy(&pi, blob.data() + info.interior_prefix_offset + 4 * count, 4);
        CHECK(pe == ne && pi == ni, "case %d view %zu: prefix", c, i);
        CHECK(f.src == v[i].src && f.dst == v[i].dst && f.width == g.sw && f.height == g.sh, "case %d view %zu: record's view", c, i);
        CHECK(f.sp32 == (uint64_t)g.rp && f.srec == (uint64_t)g.span, "case %d view %zu: read side %u %u", c, i, f.sp32, f.srec);
        CHECK(f.dp32 == g.dp && f.drec == (uint64_t)(g.sh - 1) * g.dp + g.sw, "case %d view %zu: written side", c, i);
        CHECK((f.full_x == 0) == (f.full_y == 0) && f.full_x <= g.sw / 128 && f.full_y <= g.sh / 64, "case %d view %zu: full %u x %u", c, i, f.full_x, f.full_y);
        if (g.sw >= 128 && g.sh >= 64) CHECK(f.full_x == g.sw / 128 || f.full_x == 0, "case %d view %zu: full_x", c, i);
        // the model: every interior tile is safe at every depth; without the hazard nothing is given up
        uint64_t max_off = 0;
        for (uint32_t ty = 0; ty < f.full_y; ++ty)
            for (uint32_t tx = 0; tx < f.full_x; ++tx)
                for (int nh = 1; nh <= 5; ++nh) CHECK(tile_loads_ok(f, s, tx, ty, nh, &max_off), "case %d view %zu: interior tile (%u, %u) nh %d loses bytes", c, i, tx, ty, nh);
        CHECK(max_off < (1ull << 32), "case %d view %zu: offset wraps", c, i);
        const bool hazard = (uint64_t)(g.sh - 1) * (uint64_t)g.rp + (((uint64_t)(g.sw / 128) * 128) << s) > (uint64_t)g.span;
        if (!hazard && g.sw >= 128 && g.sh >= 64) CHECK(f.full_x == g.sw / 128 && f.full_y == g.sh / 64, "case %d view %zu: interior tiles given up without a hazard", c, i);
        if (hazard && g.sw >= 128 && g.sh >= 64) {
            // the rule as the header words it
            uint32_t iy = g.sh / 64;
            while (iy > 0 && (uint64_t)(iy - 1) * 64 + 96 >= g.sh - 1) --iy;
            CHECK(f.full_y == iy && f.full_x == (iy ? g.sw / 128 : 0), "case %d view %zu: last-row rule %u x %u", c, i, f.full_x, f.full_y);
            // ... and it is needed where a given-up tile row reads the view's last row with wide loads (the rule is launch_decode_scaled's
            // and gives up every tile row that reaches as far, read or not): that row would lose a byte
            uint64_t m = 0;
            if (iy < g.sh / 64 && s <= 2 && g.sh % 64 <= 1) {
                ViewFrame t = f;
                bool lost = false;
                for (uint32_t ty = iy; ty < g.sh / 64; ++ty) lost = lost || !tile_loads_ok(t, s, g.sw / 128 - 1, ty, 5, &m);
                CHECK(lost, "case %d view %zu: the last-row rule gave up tiles that lose nothing", c, i);
            }
        }
        const uint64_t tiles = (((uint64_t)g.sw + 127) / 128) * (((uint64_t)g.sh + 63) / 64), ipf = (uint64_t)f.full_x * f.full_y;
        ne += tiles - ipf;
        ni += ipf;
        wmax = g.sw > wmax ? g.sw : wmax;
        seen.push_back(std::vector<uint8_t>((size_t)tiles, 0));
        ++count;
    }
    CHECK(info.magic == HGI_SVIEWS_MAGIC && info.shift == s && info.count == count && info.edge_tiles == ne && info.interior_tiles == ni && info.max_width == wmax,
          "case %d: info", c);
    CHECK(info.plan_bytes == views_blob_bytes(count) && sviews_info_consistent(info), "case %d: info layout", c);
    CHECK(blob[(size_t)info.plan_bytes] == 0xAB, "case %d: the plan wrote behind plan_bytes", c);
    if (!count) return;
    // the walk
    const uint64_t blocks = list_blocks(a.nedge, a.nint);
    uint64_t idle = 0;
    for (uint64_t b = 0; b < blocks; ++b) {
        const ListBlock r = view_block((uint32_t)b, a);
        if (r.idle) {
            CHECK(b >= a.nedge && b < ((a.nedge + 7u) & ~7u), "case %d: idle block outside the padding", c);
            ++idle;
            continue;
        }
        CHECK(r.frame < count, "case %d: block's frame", c);
        if (r.frame >= count) continue;
        const ViewFrame &f = a.frames[r.frame];
        const uint32_t tx = view_tiles_x(f.width), ty = view_tiles_y(f.height);
        CHECK(r.tx < tx && r.ty < ty, "case %d: block %llu -> tile (%u, %u) of %u x %u", c, (unsigned long long)b, r.tx, r.ty, tx, ty);
        if (!(r.tx < tx && r.ty < ty)) continue;
        const bool inside = r.tx < f.full_x && r.ty < f.full_y;
        CHECK(inside == !r.edge, "case %d: block %llu kind", c, (unsigned long long)b);
        uint8_t &m = seen[r.frame][(size_t)r.ty * tx + r.tx];
        CHECK(m == 0, "case %d: tile covered twice", c);
        m = 1;
    }
    CHECK(idle == ((a.nedge + 7u) & ~7u) - a.nedge, "case %d: idle blocks", c);
    for (auto &fr : seen)
        for (uint8_t m : fr) CHECK(m == 1, "case %d: tile not covered", c);
}

void one_list(int c)
{
    const size_t n = c % 16 == 15 ? 1 : (size_t)rnd_in(1, 24);
    const uint32_t s = c % 5 == 4 ? (uint32_t)rnd_in(3, 6) : (uint32_t)rnd_in(1, 2);
    std::vector<hgi_sview_pair> v(n);
    uint64_t at = (1ull << 40) + rnd_in(0, 4095);
    for (size_t i = 0; i < n; ++i) {
        uint32_t w = (uint32_t)rnd_in(0, 1500), h = (uint32_t)rnd_in(0, 1500);
        if (c % 4 == 1) {      // grids that map to whole tiles, from their smallest to their largest
            const uint32_t sw = 128 * (uint32_t)rnd_in(1, 3), sh = 64 * (uint32_t)rnd_in(1, 4) + (uint32_t)rnd_in(0, 2);
            w = ((sw - 1) << s) + 1 + (uint32_t)rnd_in(0, (1u << s) - 1);
            h = ((sh - 1) << s) + 1 + (uint32_t)rnd_in(0, (1u << s) - 1);
        }
        v[i].width = w;
        v[i].height = h;
        v[i].src_pitch = w + kGaps[rnd_in(0, 5)];
        v[i].dst_pitch = (w ? cdiv_pow2(w, s) : 0) + kGaps[rnd_in(0, 5)];
        v[i].src = at + rnd_in(0, 130);
        at = v[i].src + (uint64_t)h * v[i].src_pitch + 8 + rnd_in(0, 300);
        v[i].dst = at + rnd_in(0, 130);
        at = v[i].dst + (uint64_t)h * v[i].dst_pitch + 8 + rnd_in(0, 300);
    }
    std::vector<uint8_t> blob((size_t)views_blob_bytes(n) + 1, 0xAB);
    hgi_sviews_info info;
    memset(&info, 0, sizeof(info));
    const SViewsJudged p = sviews_plan(v.data(), n, s, blob.data(), &info);
    CHECK(p.verdict == kSViewsOk, "case %d: a list of disjoint small grids refused (%d)", c, (int)p.verdict);
    if (p.verdict != kSViewsOk) return;
    check_served(c, v, s, blob, info);
    // the launch's judgement on it
    const uint32_t r = (uint32_t)rnd_in(1, 8);
    const SViewsLaunchJudged j = sviews_judge(kPlan, &info, s + r, rnd_in(0, 1) ? HGI_INTERP_CROSSED : HGI_INTERP_LEFTTOP);
    if (info.count == 0)
        CHECK(j.verdict == kSViewsEmpty && j.status == HGI_OK, "case %d: empty plan", c);
    else
        CHECK(j.verdict == kSViewsLaunch && j.status == HGI_OK && j.k == (r < 6 ? r : 4) && j.up == (r < 6 ? 0 : r - 4) && j.text[0] == 0, "case %d: served launch r %u", c, r);
}

// ---- aliasing against marked bytes ---------------------------------------------------------------------------------------------
struct Rect {
    uint64_t lo;
    uint32_t w, h;
    uint64_t pitch;
    bool out;
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

void one_arena(int c)
{
    const uint64_t base = 1ull << 41;
    const uint32_t P = (uint32_t)rnd_in(40, 96), P2 = c % 3 == 0 ? (uint32_t)rnd_in(40, 96) : P, rows = 48;
    const uint32_t s = (uint32_t)rnd_in(1, 3);
    const size_t n = (size_t)rnd_in(1, 5);
    std::vector<uint8_t> arena((size_t)rows * 96 * 4 + 4096, 0);
    std::vector<hgi_sview_pair> v(n);
    std::vector<Rect> rc;
    for (size_t i = 0; i < n; ++i) {
        const uint32_t w = (uint32_t)rnd_in(1, 36), h = (uint32_t)rnd_in(1, 20), sw = cdiv_pow2(w, s), sh = cdiv_pow2(h, s);
        const uint32_t sp = rnd_in(0, 3) ? P : P2, dp = rnd_in(0, 3) ? P : P2;
        v[i].width = w;
        v[i].height = h;
        v[i].src_pitch = sp;
        v[i].dst_pitch = dp;
        // grids in the upper half of the arena, images mostly in the lower: some lists are served, some collide
        v[i].src = base + rnd_in(0, rows / 2) * sp + rnd_in(0, sp - w);
        v[i].dst = base + (rnd_in(0, 5) ? rows * 96 : 0) + rnd_in(0, rows / 2) * dp + rnd_in(0, dp - sw);
        rc.push_back(Rect{v[i].src, w, h, sp, false, i});
        rc.push_back(Rect{v[i].dst, sw, sh, dp, true, i});
    }
    bool oo = false, oi = false;
    for (size_t x = 0; x < rc.size(); ++x)
        for (size_t y = x + 1; y < rc.size(); ++y) {
            const Rect &a = rc[x], &b = rc[y];
            if (!a.out && !b.out) continue;
            const uint64_t ahi = a.lo + (uint64_t)(a.h - 1) * (a.h > 1 ? a.pitch : 0) + a.w, bhi = b.lo + (uint64_t)(b.h - 1) * (b.h > 1 ? b.pitch : 0) + b.w;
            if (!(a.lo < bhi && b.lo < ahi)) continue;
            const bool judged = a.h == 1 || b.h == 1 || a.pitch == b.pitch;
            const bool meet = judged ? bytes_meet(a, b, arena, base) : true;      // different pitches: refused, conservatively
            if (meet) (a.out && b.out ? oo : oi) = true;
        }
    std::vector<uint8_t> blob((size_t)views_blob_bytes(n) + 1, 0xAB);
    hgi_sviews_info info;
    memset(&info, 0, sizeof(info));
    const SViewsJudged p = sviews_plan(v.data(), n, s, blob.data(), &info);
    const SViewsVerdict want = oo ? kSViewsOutOut : oi ? kSViewsOutIn : kSViewsOk;
    CHECK(p.verdict == want, "arena %d: verdict %d, bytes say %d", c, (int)p.verdict, (int)want);
    if (p.verdict != kSViewsOk) {
        CHECK(info.magic == 0 && blob[0] == 0xAB, "arena %d: a refused plan wrote something", c);
        CHECK(p.a < n && p.b < n && (p.verdict != kSViewsOutOut || p.a < p.b), "arena %d: the pair named", c);
    } else
        check_served(c, v, s, blob, info);
}

// ---- every rule alone and in pairs -----------------------------------------------------------------------------------------------
const uint64_t A = 1ull << 42, B = 1ull << 43;
hgi_sview_pair good(int i) { return hgi_sview_pair{A + (uint64_t)i * (1ull << 30), B + (uint64_t)i * (1ull << 30), 300, 200, 320, 160}; }

// rule -> how a two-entry list (shift 1 unless the rule says otherwise) breaks it
enum Rule { rNullEntry, rSrcPitch, rDstPitch, rTiles, rOutOut, rOutIn, rShiftZero, rRead32, rWrite32, rCount };
const SViewsVerdict kWant[rCount] = {kSViewsNullEntry, kSViewsSrcPitch, kSViewsDstPitch, kSViewsTiles, kSViewsOutOut, kSViewsOutIn, kSViewsShiftZero, kSViewsRead32, kSViewsWrite32};

// breaks `r` in list `v` (entry 1 for the per-entry rules; rTiles is the giant entry that rules() puts into slot 2)
void breakit(std::vector<hgi_sview_pair> &v, uint32_t &s, Rule r)
{
    switch (r) {
    case rNullEntry: v[1].src = 0; break;
    case rSrcPitch: v[1].src_pitch = v[1].width - 1; break;
    case rDstPitch: v[1].dst_pitch = 3; break;
    case rOutOut: v[3].dst = v[0].dst ? v[0].dst + 10 : 0, v[3].dst_pitch = v[0].dst_pitch; break;
    case rOutIn: v[4].dst = v[0].src + 5, v[4].dst_pitch = v[0].src_pitch; break;
    case rShiftZero: s = 0; for (auto &e : v) e.dst_pitch = e.dst_pitch < e.width && e.dst_pitch > 3 ? e.width : e.dst_pitch; break;
    case rRead32: v[1].src_pitch = 1ull << 31; break;
    case rWrite32: v[1].dst_pitch = 1ull << 32, v[1].dst = 1ull << 50; break;      // (far from every other span: aliasing is judged first)
    default: break;
    }
}

void rules()
{
    for (int x = 0; x < rCount; ++x)
        for (int y = x; y < rCount; ++y) {
            std::vector<hgi_sview_pair> v;
            for (int i = 0; i < 5; ++i) v.push_back(good(i));
            v[2].width = 0;      // (the slot of the giant entry: empty unless rTiles)
            uint32_t s = 1;
            if ((x == rSrcPitch && y == rRead32) || (x == rDstPitch && y == rWrite32)) continue;      // one field, two values
            if (x == rTiles || y == rTiles) {
                // the giant entry: 2^49 tiles; it lies far below every other entry and is as legal as they are otherwise
                v[2] = hgi_sview_pair{1ull << 20, 1ull << 20, 0xFFFFFFFFu, 0xFFFFFFFFu, 1ull << 32, 1ull << 32};
                v[2].dst = 0xFFFFFFFF00000000ull;
            }
            breakit(v, s, (Rule)x);
            if (y != x) breakit(v, s, (Rule)y);
            std::vector<uint8_t> blob((size_t)views_blob_bytes(v.size()) + 1, 0xAB);
            hgi_sviews_info info;
            memset(&info, 0, sizeof(info));
            const SViewsJudged p = sviews_plan(v.data(), v.size(), s, blob.data(), &info);
            CHECK(p.verdict == kWant[x], "rules %d + %d: verdict %d, not the earlier rule's %d", x, y, (int)p.verdict, (int)kWant[x]);
            CHECK(info.magic == 0 && blob[0] == 0xAB, "rules %d + %d: a refused plan wrote something", x, y);
            if (x <= rDstPitch || x >= rRead32) CHECK(p.a == 1, "rules %d + %d: names view %zu", x, y, p.a);
            if (x == rOutOut) CHECK(p.a == 0 && p.b == 3, "rules %d + %d: names views %zu and %zu", x, y, p.a, p.b);
            if (x == rOutIn) CHECK(p.a == 4 && p.b == 0, "rules %d + %d: names views %zu and %zu", x, y, p.a, p.b);
        }
    // per entry the rules go in list order: an earlier entry's later rule is reported before a later entry's earlier rule
    {
        std::vector<hgi_sview_pair> v = {good(0), good(1)};
        v[0].dst_pitch = 3;
        v[1].src = 0;
        hgi_sviews_info info;
        memset(&info, 0, sizeof(info));
        std::vector<uint8_t> blob(512, 0xAB);
        const SViewsJudged p = sviews_plan(v.data(), 2, 1, blob.data(), &info);
        CHECK(p.verdict == kSViewsDstPitch && p.a == 0, "list order");
    }
    // what is not a fault: the pitch of a one-row side, overlapping grids, a view of one output row without a pitch, shift 31
    {
        std::vector<hgi_sview_pair> v = {good(0), good(1), good(2)};
        v[0].height = 1, v[0].src_pitch = 0, v[0].dst_pitch = 0;
        v[1].height = 2, v[1].dst_pitch = 0;      // sh == 1 at shift 1
        v[2].src = v[1].src + 7;                  // two grids overlap
        v[2].src_pitch = v[1].src_pitch;
        hgi_sviews_info info;
        std::vector<uint8_t> blob(512, 0xAB);
        CHECK(sviews_plan(v.data(), 3, 1, blob.data(), &info).verdict == kSViewsOk, "one-row sides");
        ViewFrame f;
        memcpy(&f, blob.data(), 64);
        CHECK(f.width == 150 && f.height == 1 && f.sp32 == 300 && f.srec == 300 && f.dp32 == 150 && f.drec == 150, "one-row grid's record");
        memcpy(&f, blob.data() + 64, 64);
        CHECK(f.height == 1 && f.sp32 == 320 + 300 && f.srec == 320 + 300, "a view of one output row reads behind its span below row 0");
        // the bound of the read side holds the columns of a whole tile, halo and chunk, at 2^s bytes each: 208 << s < 2^32 - 64 - rows
        CHECK(sviews_plan(v.data(), 3, 24, blob.data(), &info).verdict == kSViewsOk && info.shift == 24 && info.max_width == 1 && info.edge_tiles == 3, "shift 24");
        for (uint32_t s = 25; s <= 31; ++s) CHECK(sviews_plan(v.data(), 3, s, blob.data(), &info).verdict == kSViewsRead32, "shift %u", s);
    }
    // the bound of the read side, at its edge: (ty * 64 + 64) * rp + (tx * 128 + 80) * 2^s + 64 < 2^32
    for (uint32_t s = 1; s <= 3; ++s)
        for (int d = -2; d <= 2; ++d) {
            hgi_sview_pair e = good(0);
            e.width = 1000, e.height = 1001;
            const uint32_t sh = cdiv_pow2(e.height, s), ty = (sh + 63) / 64, tx = (cdiv_pow2(e.width, s) + 127) / 128;
            const uint64_t room = (1ull << 32) - 64 - ((uint64_t)(tx * 128 + 80) << s);
            e.src_pitch = ((room / (ty * 64 + 64)) >> s) + (d + 2) / 2 - 1 + (d > 0);
            e.dst_pitch = 1000;
            const Geo g = geo(e, s);
            hgi_sviews_info info;
            std::vector<uint8_t> blob(512, 0xAB);
            const SViewsJudged p = sviews_plan(&e, 1, s, blob.data(), &info);
            CHECK((p.verdict == kSViewsOk) == g.read32 && (p.verdict == kSViewsOk || p.verdict == kSViewsRead32), "read bound s %u d %d: %d", s, d, (int)p.verdict);
            if (p.verdict == kSViewsOk) {
                ViewFrame f;
                memcpy(&f, blob.data(), 64);
                uint64_t m = 0;
                tile_loads_ok(f, s, tx - 1, ty - 1, 5, &m);
                CHECK(m < (1ull << 32), "read bound s %u d %d: an offset wraps", s, d);
            }
        }
}

// ---- the launch's judgement ------------------------------------------------------------------------------------------------------
hgi_sviews_info served_info(uint32_t s)
{
    hgi_sview_pair e = good(0);
    hgi_sviews_info info;
    std::vector<uint8_t> blob(512, 0xAB);
    memset(&info, 0, sizeof(info));
    const SViewsJudged p = sviews_plan(&e, 1, s, blob.data(), &info);
    CHECK(p.verdict == kSViewsOk, "served_info");
    return info;
}

void judge()
{
    const void *odd = reinterpret_cast<const void *>((uintptr_t(1) << 40) + 8);
    hgi_sviews_info ok = served_info(2), broken = ok;
    broken.max_width = 0;
    struct Call {
        const void *d_plan;
        const hgi_sviews_info *info;
        uint32_t levels;
        int interp;      // (an int: an enumerator's value is not loaded from memory before the judgement has seen it)
    };
    const Call base = {kPlan, &ok, 6, 1};
    CHECK(sviews_judge(base.d_plan, base.info, base.levels, (hgi_interp)base.interp).verdict == kSViewsLaunch, "judge: the base call is served");
    // the rules in the header's order; each entry breaks one
    enum { jInfoNull, jInfo, jPlanNull, jPlanAlign, jLevelsRange, jInterp, jZero, jGather, jDepth, jCount };
    const SViewsLaunchVerdict want[jCount] = {kSViewsInfoNull, kSViewsInfo, kSViewsPlanNull, kSViewsPlanAlign, kSViewsLevelsRange, kSViewsInterp,
                                              kSViewsLevelsZero, kSViewsGather, kSViewsDepth};
    auto apply = [&](Call &c, int r) {
        switch (r) {
        case jInfoNull: c.info = nullptr; break;
        case jInfo: c.info = &broken; break;
        case jPlanNull: c.d_plan = nullptr; break;
        case jPlanAlign: c.d_plan = odd; break;
        case jLevelsRange: c.levels = 32; break;
        case jInterp: c.interp = 7; break;
        case jZero: c.levels = 0; break;
        case jGather: c.levels = 2; break;
        case jDepth: c.levels = 11; break;
        }
    };
    for (int x = 0; x < jCount; ++x)
        for (int y = x; y < jCount; ++y) {
            if ((x == jInfoNull && y == jInfo) || (x == jPlanNull && y == jPlanAlign)) continue;                 // one argument, two values
            if (x >= jLevelsRange && y >= jLevelsRange && x != y && x != jInterp && y != jInterp) continue;      // `levels` has one value
            Call c = base;
            apply(c, y);
            apply(c, x);
            const SViewsLaunchJudged j = sviews_judge(c.d_plan, c.info, c.levels, (hgi_interp)c.interp);
            CHECK(j.verdict == want[x] && j.status == (x < jZero ? HGI_EINVAL : HGI_EUNSUPPORTED) && j.text[0] != 0, "judge %d + %d: verdict %d status %d", x, y, (int)j.verdict, (int)j.status);
        }
    // the split of what remains, every served depth at every shift that leaves one
    for (uint32_t s = 1; s <= 24; ++s) {
        const hgi_sviews_info info = served_info(s);
        for (uint32_t levels = 0; levels <= 31; ++levels) {
            const SViewsLaunchJudged j = sviews_judge(kPlan, &info, levels, HGI_INTERP_LEFTTOP);
            if (levels == 0)
                CHECK(j.verdict == kSViewsLevelsZero, "judge: levels 0 at shift %u", s);
            else if (levels <= s)
                CHECK(j.verdict == kSViewsGather && j.status == HGI_EUNSUPPORTED, "judge: levels %u <= shift %u", levels, s);
            else if (levels - s >= 9)
                CHECK(j.verdict == kSViewsDepth && j.status == HGI_EUNSUPPORTED, "judge: levels %u - shift %u", levels, s);
            else {
                const uint32_t r = levels - s;
                CHECK(j.verdict == kSViewsLaunch && j.status == HGI_OK && j.k == (r <= 5 ? r : 4) && j.up == (r <= 5 ? 0 : r - 4), "judge: levels %u shift %u -> k %u up %u", levels, s, j.k, j.up);
            }
        }
    }
    // the empty plan is decided first, whatever the other arguments
    for (uint32_t s : {0u, 1u, 31u}) {
        hgi_sviews_info e;
        memset(&e, 0, sizeof(e));
        CHECK(sviews_plan(nullptr, 0, s, nullptr, &e).verdict == kSViewsOk && e.magic == HGI_SVIEWS_MAGIC && e.count == 0 && e.shift == s, "empty plan");
        for (uint32_t levels : {0u, 4u, 99u}) CHECK(sviews_judge(nullptr, &e, levels, (hgi_interp)-1).verdict == kSViewsEmpty, "empty plan first");
        hgi_sview_pair z[2] = {{0, 0, 0, 5, 0, 0}, {0, 0, 7, 0, 1, 1}};
        uint8_t dummy[256];
        CHECK(sviews_plan(z, 2, s, dummy, &e).verdict == kSViewsOk && e.count == 0 && e.plan_bytes == 0, "only empty entries");
    }
    // foreign magics, both ways
    for (uint32_t magic : {(uint32_t)HGI_VIEWS_MAGIC, (uint32_t)HGI_MVIEWS_MAGIC, 0u}) {
        hgi_sviews_info f = ok;
        f.magic = magic;
        CHECK(sviews_judge(kPlan, &f, 6, HGI_INTERP_CROSSED).verdict == kSViewsInfo, "judge: magic %08x accepted", magic);
        f.count = f.edge_tiles = f.interior_tiles = f.max_width = 0;
        f.plan_bytes = f.edge_prefix_offset = f.interior_prefix_offset = 0;
        CHECK(sviews_judge(kPlan, &f, 6, HGI_INTERP_CROSSED).verdict == kSViewsInfo, "judge: an empty plan of magic %08x accepted", magic);
    }
    {
        static_assert(sizeof(hgi_views_info) == sizeof(hgi_sviews_info), "hgi_views_info's layout");
        hgi_views_info theirs;
        memcpy(&theirs, &ok, sizeof(theirs));
        CHECK(!views_info_consistent(theirs), "the view lists accept this library's info");
        theirs.magic = HGI_VIEWS_MAGIC;
        CHECK(!views_info_consistent(theirs), "the view lists accept an info with a shift in the reserved slot");
        hgi_mviews_info m;
        memset(&m, 0, sizeof(m));
        memcpy(&m, &ok, sizeof(ok));
        CHECK(!mviews_info_consistent(m), "the mapped view lists accept this library's info");
        // ... and a real plan of theirs is refused here
        hgi_view_pair e = {A, B, 300, 200, 320, 320};
        std::vector<uint8_t> blob(512, 0);
        CHECK(views_plan(&e, 1, blob.data(), &theirs).verdict == kViewsOk, "their plan");
        hgi_sviews_info mine;
        memcpy(&mine, &theirs, sizeof(mine));
        CHECK(sviews_judge(kPlan, &mine, 6, HGI_INTERP_CROSSED).verdict == kSViewsInfo, "judge: the view lists' plan accepted");
    }
}

}  // namespace

int main(int argc, char **argv)
{
    const int cases = argc > 1 ? atoi(argv[1]) : 1500;
    if (argc > 2) g_x = strtoull(argv[2], nullptr, 0) | 1;
    rules();
    judge();
    for (int c = 0; c < cases; ++c) {
        one_list(c);
        one_arena(c);
    }
    std::printf("%d cases, %d failures\n", cases, g_bad);
    return g_bad ? 1 : 0;
}
