// rustyhgi_amd/qviews/hgi_qviews_plan.h -- the judgement of the requantize view lists' launch -- under ASan / UBSan, a stand-alone
// program.  The plan of a list is the view lists' own (views_plan), run here as it stands:
//   * random small lists (1 ... 40 entries, sides 0 ... 700, pitches w + gap on each side) go through views_plan and then
//     through qviews_judge with a random served depth, interpolator and table: a served plan is served, its split of the pyramid
//     is split_levels', and view_args of the blob gives the block count the launcher will use -- every tile of every non-empty
//     grid, the ragged ones padded to eight; a list views_plan refuses (the page rule) leaves an info no launch accepts;
//   * every rule of the launch fires alone, with its status, its verdict and a message; adjacent rules fire in pairs, and the
//     earlier one is reported: the order of include/hgi_qviews.h;
//   * the empty plan is decided first, whatever the other arguments; an info of the mapped or the typed view lists' magic is
//     refused;
//   * the identity table is refused only behind every HGI_EINVAL rule and behind the depth rule; a table that differs from the
//     identity in one entry (0, 128, 255) is served.
// Nothing here touches grid memory: d_plan is judged as an address.  Usage: test_qviews_plan [lists] [seed]
#include <cstring>

#include "../../include/hgi_mviews.h"
#include "../../include/hgi_tviews.h"
#include "../../rustyhgi_amd/qviews/hgi_qviews_plan.h"
#include "plan_test_util.h"

using namespace hgi;

namespace {

const uint32_t kGaps[6] = {0, 1, 3, 16, 61, 128};
const uint32_t kMViewsMagic = HGI_MVIEWS_MAGIC, kTViewsMagic = HGI_TVIEWS_MAGIC;

bool page_rule(const hgi_view_pair &v)      // include/hgi_views.h, restated
{
    if (v.width % 4 == 0) return true;
    const uint64_t end = v.src + (uint64_t)(v.height - 1) * (v.height > 1 ? v.src_pitch : v.width) + v.width;
    return ((end - 1) >> 12) == ((end + 2) >> 12);
}

uint8_t g_ident[256], g_medium[256];
const void *const kPlan = reinterpret_cast<const void *>(uintptr_t(1) << 40);      // an address, never read

void tables()
{
    for (int i = 0; i < 256; ++i) {
        g_ident[i] = (uint8_t)i;
        g_medium[i] = (uint8_t)(i / 8 * 8 + 4 > 255 ? 255 : i / 8 * 8 + 4);
    }
}

void one_list(int c)
{
    const size_t n = c % 16 == 15 ? 1 : (size_t)rnd_in(1, 40);
    std::vector<hgi_view_pair> v(n);
    uint64_t at = (1ull << 40) + rnd_in(0, 4095);
    for (size_t i = 0; i < n; ++i) {
        uint32_t w = (uint32_t)rnd_in(0, 700), h = (uint32_t)rnd_in(0, 700);
        if (c % 16 == 14) w = 128 * (uint32_t)rnd_in(1, 5), h = 64 * (uint32_t)rnd_in(1, 6);
        v[i].width = w;
        v[i].height = h;
        v[i].src_pitch = w + kGaps[rnd_in(0, 5)];
        v[i].dst_pitch = w + kGaps[rnd_in(0, 5)];
        v[i].src = at + rnd_in(0, 130);
        if (c % 8 == 3 && w && h && w % 4) {      // some grids end on a page boundary
            const uint64_t end = v[i].src + (uint64_t)(h - 1) * (h > 1 ? v[i].src_pitch : w) + w;
            v[i].src += (4096 - end % 4096) % 4096;
        }
        at = v[i].src + (uint64_t)h * v[i].src_pitch + 8 + rnd_in(0, 300);
        v[i].dst = at + rnd_in(0, 130);
        at = v[i].dst + (uint64_t)h * v[i].dst_pitch + 8 + rnd_in(0, 300);
    }
    std::vector<uint8_t> blob((size_t)views_blob_bytes(n) + 1, 0xAB);
    hgi_views_info info;
    memset(&info, 0, sizeof(info));
    const ViewsJudged p = views_plan(v.data(), n, blob.data(), &info);
    const uint32_t levels = (uint32_t)rnd_in(1, 8);
    const hgi_interp interp = rnd_in(0, 1) ? HGI_INTERP_CROSSED : HGI_INTERP_LEFTTOP;
    uint8_t lut[256];
    for (int i = 0; i < 256; ++i) lut[i] = (uint8_t)rnd_in(0, 255);
    lut[7] = 8;      // (never the identity)
    bool tail = false;
    uint64_t tiles = 0, ne = 0, ni = 0, count = 0;
    for (size_t i = 0; i < n; ++i) {
        if (!v[i].width || !v[i].height) continue;
        tail = tail || !page_rule(v[i]);
        const uint64_t tx = (v[i].width + 127) / 128, ty = (v[i].height + 63) / 64, fx = v[i].width / 128, fy = v[i].height / 64;
        tiles += tx * ty;
        ni += fx * fy;
        ne += tx * ty - fx * fy;
        ++count;
    }
    if (tail) {
        // what the plan refuses leaves the zeroed info, and no launch accepts that
        CHECK(p.verdict == kViewsTail && info.magic == 0, "list %d: the page rule, verdict %d", c, (int)p.verdict);
        const QViewsJudged j = qviews_judge(kPlan, &info, levels, interp, lut);
        CHECK(j.status == HGI_EINVAL && j.verdict == kQViewsInfo && j.text[0], "list %d: a refused plan's info is refused", c);
        return;
    }
    CHECK(p.verdict == kViewsOk, "list %d: verdict %d at %zu", c, (int)p.verdict, p.a);
    if (p.verdict != kViewsOk) return;
    const QViewsJudged j = qviews_judge(kPlan, &info, levels, interp, lut);
    if (count == 0) {
        CHECK(j.status == HGI_OK && j.verdict == kQViewsEmpty, "list %d: only empty entries", c);
        return;
    }
    CHECK(j.status == HGI_OK && j.verdict == kQViewsLaunch && j.text[0] == 0, "list %d: a served plan, status %d verdict %d (%s)", c, (int)j.status,
          (int)j.verdict, j.text);
    uint32_t k, up;
    split_levels(levels, &k, &up);
    CHECK(j.k == k && j.up == up && j.k >= 1 && j.k <= 5 && (up == 0 || (j.k == 4 && up == levels - 4 && up <= 4)), "list %d: levels %u -> k %u up %u", c,
          levels, j.k, j.up);
    // the block count the launcher will use (views_tile_launch): list_blocks of the arrays' two totals
    const ViewArgs a = view_args(blob.data(), info);
    CHECK(a.count == count && a.nedge == ne && a.nint == ni && ne + ni == tiles, "list %d: %u frames, %u + %u tiles", c, a.count, a.nedge, a.nint);
    const uint64_t blocks = list_blocks(a.nedge, a.nint);
    CHECK(blocks == ((ne + 7) & ~(uint64_t)7) + ni && blocks != 0 && blocks + 8 < (1ull << 31), "list %d: %llu blocks", c, (unsigned long long)blocks);
    uint64_t live = 0;
    for (uint64_t b = 0; b < blocks; ++b) live += view_block((uint32_t)b, a).idle ? 0 : 1;
    CHECK(live == tiles, "list %d: %llu blocks with a tile, %llu tiles", c, (unsigned long long)live, (unsigned long long)tiles);
    CHECK(reinterpret_cast<const uint8_t *>(a.frames) == blob.data() && reinterpret_cast<const uint8_t *>(a.ipre) + 4 * count <= blob.data() + info.plan_bytes,
          "list %d: the arrays lie in the blob", c);
    // the same plan at the depths and under the table the launch does not serve
    CHECK(qviews_judge(kPlan, &info, 0, interp, lut).verdict == kQViewsLevels && qviews_judge(kPlan, &info, 9 + (uint32_t)rnd_in(0, 22), interp, lut).verdict == kQViewsLevels,
          "list %d: depth", c);
    CHECK(qviews_judge(kPlan, &info, levels, interp, g_ident).verdict == kQViewsIdentity, "list %d: identity", c);
}

// what a rule gives when it fires
struct Want {
    hgi_status status;
    QViewsVerdict verdict;
};

void rules()
{
    const hgi_view_pair one = {1ull << 50, 2ull << 50, 300, 200, 320, 301};
    std::vector<uint8_t> blob((size_t)views_blob_bytes(1));
    hgi_views_info good;
    CHECK(views_plan(&one, 1, blob.data(), &good).verdict == kViewsOk && views_info_consistent(good), "the plan of one grid");
    hgi_views_info damaged = good;
    damaged.plan_bytes += 16;
    const void *const odd = reinterpret_cast<const void *>((uintptr_t(1) << 40) + 8);

    // a call as the rules see it; rule r of `rules` broken by break_rule(r)
    struct Call {
        const void *d_plan;
        const hgi_views_info *info;
        uint32_t levels;
        int interp;
        const uint8_t *lut;
    };
    const Call served = {kPlan, &good, 4, 1, g_medium};
    const int kRules = 9;
    const Want want[kRules] = {{HGI_EINVAL, kQViewsInfoNull},  {HGI_EINVAL, kQViewsInfo},        {HGI_EINVAL, kQViewsPlanNull},
                               {HGI_EINVAL, kQViewsPlanAlign}, {HGI_EINVAL, kQViewsLutNull},     {HGI_EINVAL, kQViewsLevelsRange},
                               {HGI_EINVAL, kQViewsInterp},    {HGI_EUNSUPPORTED, kQViewsLevels}, {HGI_EUNSUPPORTED, kQViewsIdentity}};
    auto break_rule = [&](Call &c, int r) {
        switch (r) {
        case 0: c.info = nullptr; break;
        case 1: c.info = &damaged; break;
        case 2: c.d_plan = nullptr; break;
        case 3: c.d_plan = odd; break;
        case 4: c.lut = nullptr; break;
        case 5: c.levels = 32; break;
        case 6: c.interp = 2; break;
        case 7: c.levels = 9; break;
        case 8: c.lut = g_ident; break;
        }
    };
    auto compatible = [](int a, int b) {      // two breaks of one argument do not combine
        const int arg[9] = {0, 0, 1, 1, 2, 3, 4, 3, 2};
        return arg[a] != arg[b];
    };
    auto judge = [](const Call &c) { return qviews_judge(c.d_plan, c.info, c.levels, (hgi_interp)c.interp, c.lut); };
    {
        const QViewsJudged j = judge(served);
        CHECK(j.status == HGI_OK && j.verdict == kQViewsLaunch && j.k == 4 && j.up == 0 && j.text[0] == 0, "the served call");
    }
    // every rule alone
    for (int r = 0; r < kRules; ++r) {
        Call c = served;
        break_rule(c, r);
        const QViewsJudged j = judge(c);
        CHECK(j.status == want[r].status && j.verdict == want[r].verdict && j.text[0] != 0 && strlen(j.text) < sizeof(j.text) - 1, "rule %d alone: status %d verdict %d (%s)", r,
              (int)j.status, (int)j.verdict, j.text);
    }
    // every pair of rules that can be broken together -- the adjacent ones among them: the earlier one is reported
    int pairs = 0, adjacent = 0;
    for (int r = 0; r < kRules; ++r)
        for (int s = r + 1; s < kRules; ++s) {
            if (!compatible(r, s)) continue;
            Call c = served;
            break_rule(c, r);
            break_rule(c, s);
            const QViewsJudged j = judge(c);
            CHECK(j.status == want[r].status && j.verdict == want[r].verdict, "rules %d and %d: verdict %d", r, s, (int)j.verdict);
            ++pairs;
            adjacent += s == r + 1 ? 1 : 0;
        }
    // (0 | 1, 2 | 3, 4 | 8 and 5 | 7 break one argument in two ways and cannot stand together: 36 - 4 pairs, 8 - 2 adjacent ones)
    CHECK(pairs == 32 && adjacent == 6, "%d pairs, %d adjacent", pairs, adjacent);
    // levels: 0 and 9 ... 31 are unsupported, 32 and more invalid; 1 ... 8 split as the other lists split them
    for (uint32_t levels = 0; levels <= 40; ++levels) {
        Call c = served;
        c.levels = levels;
        const QViewsJudged j = judge(c);
        const QViewsVerdict w = levels > 31 ? kQViewsLevelsRange : levels == 0 || levels > 8 ? kQViewsLevels : kQViewsLaunch;
        CHECK(j.verdict == w && (w != kQViewsLaunch || (j.k == (levels < 6 ? levels : 4) && j.up == (levels < 6 ? 0 : levels - 4))), "levels %u: verdict %d", levels,
              (int)j.verdict);
    }
    for (int interp : {-1, 2, 7, 1 << 30}) {
        Call c = served;
        c.interp = interp;
        CHECK(judge(c).verdict == kQViewsInterp, "interpolator %d", interp);
    }
    for (uintptr_t off = 1; off < 16; ++off)
        CHECK(qviews_judge(reinterpret_cast<const void *>((uintptr_t(1) << 40) + off), &good, 4, HGI_INTERP_CROSSED, g_medium).verdict == kQViewsPlanAlign, "d_plan + %d", (int)off);
    // the identity table: behind every HGI_EINVAL rule and behind the depth rule (the pairs above); one entry off is served
    for (int at : {0, 128, 255}) {
        uint8_t lut[256];
        memcpy(lut, g_ident, 256);
        lut[at] ^= 1;
        CHECK(!qviews_identity(lut) && qviews_judge(kPlan, &good, 4, HGI_INTERP_LEFTTOP, lut).verdict == kQViewsLaunch, "the identity but for entry %d", at);
        lut[at] ^= 1;
        CHECK(qviews_identity(lut) && qviews_judge(kPlan, &good, 4, HGI_INTERP_LEFTTOP, lut).verdict == kQViewsIdentity, "the identity");
    }
    for (uint32_t levels : {0u, 9u, 31u}) CHECK(qviews_judge(kPlan, &good, levels, HGI_INTERP_CROSSED, g_ident).verdict == kQViewsLevels, "depth before the table");
    // the infos of the sibling lists: their magic is not the view lists'
    for (uint32_t magic : {kMViewsMagic, kTViewsMagic, 0u}) {
        hgi_views_info other = good;
        other.magic = magic;
        const QViewsJudged j = qviews_judge(kPlan, &other, 4, HGI_INTERP_CROSSED, g_medium);
        CHECK(magic != HGI_VIEWS_MAGIC && j.status == HGI_EINVAL && j.verdict == kQViewsInfo, "magic %08x", magic);
        other.count = other.edge_tiles = other.interior_tiles = other.max_width = 0;      // ... nor as an empty plan
        other.plan_bytes = other.edge_prefix_offset = other.interior_prefix_offset = 0;
        CHECK(qviews_judge(kPlan, &other, 4, HGI_INTERP_CROSSED, g_medium).verdict == kQViewsInfo, "magic %08x on an empty plan", magic);
    }
    hgi_views_info d = good;
    d.reserved = 4;      // (where the sibling infos keep their element size)
    CHECK(qviews_judge(kPlan, &d, 4, HGI_INTERP_CROSSED, g_medium).verdict == kQViewsInfo, "a reserved word that is set");
    // the empty plans: decided first, whatever the other arguments
    const hgi_view_pair skipped[2] = {{0, 0, 0, 9, 0, 0}, {0, 0, 7, 0, 1, 1}};
    for (size_t n : {size_t(0), size_t(2)}) {
        hgi_views_info e;
        CHECK(views_plan(skipped, n, nullptr, &e).verdict == kViewsOk && e.count == 0 && e.magic == HGI_VIEWS_MAGIC, "a plan of no frame");
        for (int r = 2; r < kRules; ++r) {
            Call c = served;
            c.info = &e;
            break_rule(c, r);
            const QViewsJudged j = judge(c);
            CHECK(j.status == HGI_OK && j.verdict == kQViewsEmpty && j.text[0] == 0, "the empty plan with rule %d broken", r);
        }
        const QViewsJudged j = qviews_judge(nullptr, &e, 99, (hgi_interp)-1, nullptr);
        CHECK(j.status == HGI_OK && j.verdict == kQViewsEmpty, "the empty plan with nothing else");
    }
}

}  // namespace

int main(int argc, char **argv)
{
    const int cases = argc > 1 ? atoi(argv[1]) : 2000;
    if (argc > 2) g_x = strtoull(argv[2], nullptr, 0) | 1u;
    tables();
    for (int c = 0; c < cases; ++c) one_list(c);
    rules();
    std::printf("qviews plan: %d cases, %d failures\n", cases, g_bad);
    return g_bad ? 1 : 0;
}
