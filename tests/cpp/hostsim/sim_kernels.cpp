// The launch_* functions of csrc/hgi_kernels.h as plain CPU code on the simulated runtime (hostsim.cpp), written from that
// header's contracts and the level restatement of ref_levels.h -- not from the kernels.  Each launch is queued on its stream and
// runs when the schedule executes it.  It aborts when its arguments leave the ranges the header states (k against the tile
// depth of the _16 / _32 / _64 build, up <= 4, the seed planes' shape ...), and it reads and writes exactly the bytes the
// contract allows -- w * h per frame at the frame stride, sw * sh per seed plane, the width bytes of each output row -- each
// range checked against the live device blocks, so that scratch sizing and slot arithmetic are checked against use.
//
// A row-limited launch (the bands of host_banded) keeps the rows below row_limit of the code of the whole row-shifted view.
// Those rows depend on the view's rows 0 ... row_limit + 2^k inclusive and on nothing below (a prediction reads the corners of
// its own 2^(s + 1) cell, s < k, and row_limit is a multiple of 2^k), so the launch codes that prefix of the view: it reads
// every byte the kept rows mathematically depend on, uploaded or not.  This checks the host's upload plan against the
// dependency; it does not check the real kernels' read set (that stays with the HGI_TEST_BAND_HOLD GPU test).
#include <string.h>

#include <vector>

#include "../../../rustyhgi_amd/csrc/hgi_framelist.h"
#include "../../../rustyhgi_amd/csrc/hgi_kernels.h"
#include "../../../rustyhgi_amd/csrc/hgi_knobs.h"
#include "../../../rustyhgi_amd/csrc/hgi_pitched.h"
#include "hostsim.h"
#include "ref_levels.h"

extern "C" int hgi_oracle_synth(int kind, uint64_t seed, uint64_t frame, uint32_t w, uint32_t h, uint8_t *out);

namespace hgi {

namespace {

typedef std::vector<uint8_t> Bytes;

struct Table {
    uint8_t v[256];
};

Table unpack(const Lut256 &l, bool ident, const char *name)
{
    Table t;
    memcpy(t.v, l.w, 256);
    bool is = true;
    for (int i = 0; i < 256; ++i) is = is && t.v[i] == i;
    if (is != ident) sim::die("%s: lut_is_identity = %d contradicts the table", name, (int)ident);
    return t;
}

uint32_t ceil_shift(uint32_t v, uint32_t k) { return (uint32_t)((((uint64_t)v - 1) >> k) + 1); }

// The pyramid depth K a tile launch codes and whether planes seed it; aborts on arguments outside the header's ranges.
struct Depth {
    uint32_t K;
    bool planes;
};

Depth check_depth(const char *name, bool has, const Seeds &sd, uint32_t k, uint32_t maxk, uint32_t w, uint32_t h, uint32_t batch, bool encode,
                  int interp)
{
    if (interp != kInterpLeftTop && interp != kInterpCrossed) sim::die("%s: interpolator %d", name, interp);
    if (w == 0 || h == 0 || batch == 0) sim::die("%s: empty launch %u x %u x %u", name, w, h, batch);
    if (k < 1 || k > maxk) sim::die("%s: k = %u outside 1 ... %u", name, k, maxk);
    if (!has) return {k, false};
    if (sd.up > 4) sim::die("%s: up = %u > 4", name, sd.up);
    if (sd.up && k != 4) sim::die("%s: the cone needs k == 4, got %u", name, k);
    if (!sd.up && !sd.rec) sim::die("%s: seeds with up == 0 and no planes", name);
    if (!sd.up && k < (uint32_t)kSeededMinLevels) sim::die("%s: a seeded launch needs k >= %d, got %u", name, kSeededMinLevels, k);
    if (!sd.rec) return {k + sd.up, false};
    const uint32_t K = k + sd.up;
    if (sd.sw != ceil_shift(w, K) || sd.sh != ceil_shift(h, K))
        sim::die("%s: seed planes %u x %u, the stride-2^%u lattice of %u x %u is %u x %u", name, sd.sw, sd.sh, K, w, h, ceil_shift(w, K), ceil_shift(h, K));
    if (batch > 1 && sd.stride < (uint64_t)sd.sw * sd.sh) sim::die("%s: seed plane stride %llu < sw * sh", name, (unsigned long long)sd.stride);
    if (encode && !sd.q) sim::die("%s: an encode on planes needs the residual plane", name);
    return {K, true};
}

// One compact w x h view coded at K levels: in -> out.  Planes (frame-local pointers, rows sw bytes apart) hold the stride-2^K
// lattice when given.
void code_view(bool encode, const uint8_t *in, uint8_t *out, uint32_t w, uint32_t h, uint32_t K, int interp, const uint8_t *lut, const uint8_t *rec_pl,
               const uint8_t *q_pl, uint32_t sw)
{
    Bytes recv;
    uint8_t *rec = out;   // decoding: the image is its own reconstruction
    if (encode) {
        recv.assign(in, in + (size_t)w * h);
        rec = recv.data();
    }
    if (rec_pl) {
        for (uint64_t Y = 0; (Y << K) < h; ++Y)
            for (uint64_t X = 0; (X << K) < w; ++X) {
                const size_t i = (Y << K) * w + (X << K);
                rec[i] = rec_pl[Y * sw + X];
                if (encode) out[i] = q_pl[Y * sw + X];
            }
    } else {
        ref::seed(in, out, w, h, K);
    }
    for (uint32_t s = K; s-- > 0;) {
        if (encode) ref::encode_level(rec, out, w, h, s, interp, lut);
        else ref::decode_level(in, out, w, h, s, interp);
    }
}

hipError_t fused(const char *name, bool encode, uint32_t maxk, const uint8_t *in, uint8_t *out, const Frames &f, uint32_t k, int interp, const Lut256 &lut,
                 bool ident, const Seeds *seeds, hipStream_t s, uint32_t row_limit, int resident_tiles)
{
    const bool has = seeds != nullptr;
    const Seeds sd = has ? *seeds : Seeds{};
    const Frames fr = f;
    const Lut256 l = lut;
    sim::launch(s, name, [=]() {
        const Depth d = check_depth(name, has, sd, k, maxk, fr.width, fr.height, fr.batch, encode, interp);
        if (row_limit % 64) sim::die("%s: row_limit %u is no multiple of 64", name, row_limit);
        if (resident_tiles < -1) sim::die("%s: resident_tiles %d", name, resident_tiles);
        const Table t = encode ? unpack(l, ident, name) : Table{};
        const uint32_t w = fr.width, h = fr.height;
        const size_t n = (size_t)w * h;
        if (fr.batch > 1 && fr.frame_stride < n) sim::die("%s: frame stride < w * h", name);
        const uint32_t rows = row_limit && row_limit < h ? row_limit : h;
        uint64_t hv = h;
        if (rows < h && (uint64_t)rows + ((uint64_t)1 << d.K) + 1 < h) hv = (uint64_t)rows + ((uint64_t)1 << d.K) + 1;
        Bytes tmp;
        for (uint32_t b = 0; b < fr.batch; ++b) {
            const uint8_t *src = in + b * fr.frame_stride;
            uint8_t *dst = out + b * fr.frame_stride;
            sim::dev_check(src, n, name);
            sim::dev_check(dst, (size_t)rows * w, name);
            const uint8_t *rp = nullptr, *qp = nullptr;
            if (d.planes) {
                rp = sd.rec + b * sd.stride;
                sim::dev_check(rp, (size_t)sd.sw * sd.sh, name);
                if (encode) {
                    qp = sd.q + b * sd.stride;
                    sim::dev_check(qp, (size_t)sd.sw * sd.sh, name);
                }
            }
            if (rows == h) {
                code_view(encode, src, dst, w, h, d.K, interp, t.v, rp, qp, sd.sw);
            } else {
                tmp.resize((size_t)hv * w);
                code_view(encode, src, tmp.data(), w, (uint32_t)hv, d.K, interp, t.v, rp, qp, sd.sw);
                memcpy(dst, tmp.data(), (size_t)rows * w);
            }
        }
    });
    return hipSuccess;
}

// rows `pitch` apart -> a compact plane, reading the width bytes of each row
Bytes gather_rows(const uint8_t *p, uint64_t pitch, uint32_t w, uint32_t h, const char *name)
{
    sim::dev_check(p, (size_t)(h - 1) * (h > 1 ? pitch : 0) + w, name);
    Bytes v((size_t)w * h);
    for (uint32_t y = 0; y < h; ++y) memcpy(v.data() + (size_t)y * w, p + (size_t)y * (h > 1 ? pitch : 0), w);
    return v;
}

void scatter_rows(const uint8_t *v, uint32_t vw, uint32_t x0, uint32_t y0, uint8_t *p, uint64_t pitch, uint32_t w, uint32_t h, const char *name)
{
    sim::dev_check(p, (size_t)(h - 1) * (h > 1 ? pitch : 0) + w, name);
    for (uint32_t y = 0; y < h; ++y) memcpy(p + (size_t)y * (h > 1 ? pitch : 0), v + (size_t)(y0 + y) * vw + x0, w);
}

struct PlanePtrs {
    const uint8_t *rec, *q;
};

PlanePtrs planes_of(const Depth &d, const Seeds &sd, uint32_t b, bool encode, const char *name)
{
    PlanePtrs p = {nullptr, nullptr};
    if (!d.planes) return p;
    p.rec = sd.rec + b * sd.stride;
    sim::dev_check(p.rec, (size_t)sd.sw * sd.sh, name);
    if (encode) {
        p.q = sd.q + b * sd.stride;
        sim::dev_check(p.q, (size_t)sd.sw * sd.sh, name);
    }
    return p;
}

hipError_t pitched(const char *name, bool encode, const uint8_t *in, uint8_t *out, const PitchedFrames &f, uint32_t k, int interp, const Lut256 &lut,
                   bool ident, const Seeds *seeds, hipStream_t s)
{
    const bool has = seeds != nullptr;
    const Seeds sd = has ? *seeds : Seeds{};
    const PitchedFrames pf = f;
    const Lut256 l = lut;
    sim::launch(s, name, [=]() {
        const Depth d = check_depth(name, has, sd, k, kFusedMaxLevels, pf.width, pf.height, pf.batch, encode, interp);
        if (pf.height > 1 && (pf.src_pitch < pf.width || pf.dst_pitch < pf.width)) sim::die("%s: pitch < width", name);
        const Table t = encode ? unpack(l, ident, name) : Table{};
        for (uint32_t b = 0; b < pf.batch; ++b) {
            const Bytes src = gather_rows(in + b * (pf.batch > 1 ? pf.src_stride : 0), pf.src_pitch, pf.width, pf.height, name);
            Bytes dst(src.size());
            const PlanePtrs p = planes_of(d, sd, b, encode, name);
            code_view(encode, src.data(), dst.data(), pf.width, pf.height, d.K, interp, t.v, p.rec, p.q, sd.sw);
            scatter_rows(dst.data(), pf.width, 0, 0, out + b * (pf.batch > 1 ? pf.dst_stride : 0), pf.dst_pitch, pf.width, pf.height, name);
        }
    });
    return hipSuccess;
}

}  // namespace

#define HGI_DEFINE_FUSED(TH, MAXK)                                                                                                      \
    hipError_t launch_decode_fused_##TH(const uint8_t *grid, uint8_t *img, const Frames &f, uint32_t k, int interp, const Seeds *seeds, \
                                        hipStream_t s, uint32_t row_limit, int resident_tiles)                                          \
    {                                                                                                                                   \
        return fused("launch_decode_fused_" #TH, false, MAXK, grid, img, f, k, interp, Lut256{}, false, seeds, s, row_limit, resident_tiles); \
    }                                                                                                                                   \
    hipError_t launch_encode_fused_##TH(const uint8_t *img, uint8_t *grid, const Frames &f, uint32_t k, int interp, const Lut256 &lut,  \
                                        bool lut_is_identity, const Seeds *seeds, hipStream_t s, uint32_t row_limit)                    \
    {                                                                                                                                   \
        return fused("launch_encode_fused_" #TH, true, MAXK, img, grid, f, k, interp, lut, lut_is_identity, seeds, s, row_limit, -1);   \
    }
HGI_DEFINE_FUSED(64, kFusedMaxLevels)
HGI_DEFINE_FUSED(32, kFusedMaxLevelsSmall)
HGI_DEFINE_FUSED(16, kFusedMaxLevelsTiny)
#undef HGI_DEFINE_FUSED

hipError_t launch_decode_region(const uint8_t *grid, uint8_t *out, const Frames &f, const RegionRect &r, uint32_t k, int interp, const Seeds *seeds,
                                hipStream_t s)
{
    static const char *name = "launch_decode_region";
    const bool has = seeds != nullptr;
    const Seeds sd = has ? *seeds : Seeds{};
    const Frames fr = f;
    const RegionRect rr = r;
    sim::launch(s, name, [=]() {
        const Depth d = check_depth(name, has, sd, k, kFusedMaxLevels, fr.width, fr.height, fr.batch, false, interp);
        if (!rr.width || !rr.height || (uint64_t)rr.x0 + rr.width > fr.width || (uint64_t)rr.y0 + rr.height > fr.height)
            sim::die("%s: window %u,%u %ux%u outside %u x %u", name, rr.x0, rr.y0, rr.width, rr.height, fr.width, fr.height);
        if (rr.height > 1 && rr.out_pitch < rr.width) sim::die("%s: out_pitch < window width", name);
        const size_t n = (size_t)fr.width * fr.height;
        Bytes img(n);
        for (uint32_t b = 0; b < fr.batch; ++b) {
            const uint8_t *src = grid + b * fr.frame_stride;
            sim::dev_check(src, n, name);
            const PlanePtrs p = planes_of(d, sd, b, false, name);
            code_view(false, src, img.data(), fr.width, fr.height, d.K, interp, nullptr, p.rec, nullptr, sd.sw);
            scatter_rows(img.data(), fr.width, rr.x0, rr.y0, out + b * rr.out_frame_stride, rr.out_pitch, rr.width, rr.height, name);
        }
    });
    return hipSuccess;
}

hipError_t launch_decode_scaled(const uint8_t *src, uint8_t *out, const ScaledView &v, uint32_t k, int interp, const Seeds *seeds, hipStream_t s)
{
    static const char *name = "launch_decode_scaled";
    const bool has = seeds != nullptr;
    const Seeds sd = has ? *seeds : Seeds{};
    const ScaledView sv = v;
    sim::launch(s, name, [=]() {
        const Depth d = check_depth(name, has, sd, k, kFusedMaxLevels, sv.width, sv.height, sv.batch, false, interp);
        if (sv.shift > 31) sim::die("%s: shift %u", name, sv.shift);
        if (sv.height > 1 && sv.out_pitch < sv.width) sim::die("%s: out_pitch < view width", name);
        const size_t n = (size_t)sv.width * sv.height;
        Bytes g(n), img(n);
        for (uint32_t b = 0; b < sv.batch; ++b) {
            const uint8_t *fp = src + b * sv.frame_stride;
            sim::dev_check(fp, sv.frame_bytes, name);
            for (uint32_t y = 0; y < sv.height; ++y)
                for (uint32_t x = 0; x < sv.width; ++x) {
                    const uint64_t off = (uint64_t)y * sv.row_pitch + ((uint64_t)x << sv.shift);
                    if (off >= sv.frame_bytes) sim::die("%s: view byte (%u, %u) lies outside frame_bytes", name, x, y);
                    g[(size_t)y * sv.width + x] = fp[off];
                }
            const PlanePtrs p = planes_of(d, sd, b, false, name);
            code_view(false, g.data(), img.data(), sv.width, sv.height, d.K, interp, nullptr, p.rec, nullptr, sd.sw);
            scatter_rows(img.data(), sv.width, 0, 0, out + b * sv.out_frame_stride, sv.out_pitch, sv.width, sv.height, name);
        }
    });
    return hipSuccess;
}

hipError_t launch_gather_view(const uint8_t *src, uint64_t src_stride, uint64_t row_pitch, uint32_t ky, uint32_t kx, uint32_t sw, uint32_t sh,
                              uint8_t *dst, uint64_t dst_pitch, uint64_t dst_stride, uint32_t batch, hipStream_t s)
{
    static const char *name = "launch_gather_view";
    sim::launch(s, name, [=]() {
        if (!sw || !sh || !batch || ky > 63 || kx > 63 || dst_pitch < sw) sim::die("%s: arguments", name);
        for (uint32_t b = 0; b < batch; ++b) {
            const uint8_t *fp = src + b * src_stride;
            uint8_t *dp = dst + b * dst_stride;
            sim::dev_check(fp, (size_t)(((uint64_t)(sh - 1) << ky) * row_pitch + ((uint64_t)(sw - 1) << kx) + 1), name);
            sim::dev_check(dp, (size_t)(sh - 1) * dst_pitch + sw, name);
            for (uint32_t y = 0; y < sh; ++y)
                for (uint32_t x = 0; x < sw; ++x) dp[(size_t)y * dst_pitch + x] = fp[((uint64_t)y << ky) * row_pitch + ((uint64_t)x << kx)];
        }
    });
    return hipSuccess;
}

namespace {

hipError_t list(const char *name, bool encode, const ListArgs &a, uint32_t k, int interp, const Lut256 &lut, bool ident, const Seeds *seeds, hipStream_t s)
{
    const bool has = seeds != nullptr;
    const Seeds sd = has ? *seeds : Seeds{};
    const ListArgs la = a;
    const Lut256 l = lut;
    sim::launch(s, name, [=]() {
        if (has && sd.rec) sim::die("%s: a list launch takes no seed planes", name);
        if (!la.count) sim::die("%s: empty list", name);
        const Table t = encode ? unpack(l, ident, name) : Table{};
        sim::dev_check(la.frames, la.count * sizeof(ListFrame), name);
        sim::dev_check(la.epre, la.count * sizeof(uint32_t), name);
        sim::dev_check(la.ipre, la.count * sizeof(uint32_t), name);
        uint32_t ne = 0, ni = 0;
        for (uint32_t i = 0; i < la.count; ++i) {
            const ListFrame F = la.frames[i];
            const Depth d = check_depth(name, has, sd, k, kFusedMaxLevels, F.width, F.height, 1, encode, interp);
            // the frame's 128 x 64 tiles, restated here (not the library's list_frame): all of them; those that lie entirely inside
            // the image, when the plan takes the check-free path for them (both counts then, or neither)
            const uint32_t tx = (uint32_t)(((uint64_t)F.width + 127) / 128), ty = (uint32_t)(((uint64_t)F.height + 63) / 64);
            const bool interior = F.full_x || F.full_y;
            if (F.tiles_x != tx || F.tiles_y != ty || (interior && (F.full_x != F.width / 128 || F.full_y != F.height / 64 || !F.full_x || !F.full_y)) ||
                F.epf != tx * ty - F.full_x * F.full_y || la.epre[i] != ne || la.ipre[i] != ni)
                sim::die("%s: frame %u of the table contradicts its shape or the prefix arrays", name, i);
            ne += F.epf;
            ni += F.full_x * F.full_y;
            const size_t n = (size_t)F.width * F.height;
            const uint8_t *src = reinterpret_cast<const uint8_t *>(F.src);
            uint8_t *dst = reinterpret_cast<uint8_t *>(F.dst);
            sim::dev_check(src, n, name);
            sim::dev_check(dst, n, name);
            code_view(encode, src, dst, F.width, F.height, d.K, interp, t.v, nullptr, nullptr, 0);
        }
        if (ne != la.nedge || ni != la.nint) sim::die("%s: nedge / nint contradict the table", name);
    });
    return hipSuccess;
}

}  // namespace

hipError_t launch_decode_list(const ListArgs &a, uint32_t max_width, uint32_t k, int interp, const Seeds *seeds, hipStream_t s)
{
    if (!max_width) sim::die("launch_decode_list: max_width 0");
    return list("launch_decode_list", false, a, k, interp, Lut256{}, false, seeds, s);
}

hipError_t launch_encode_list(const ListArgs &a, uint32_t k, int interp, const Lut256 &lut, bool ident, const Seeds *seeds, hipStream_t s)
{
    return list("launch_encode_list", true, a, k, interp, lut, ident, seeds, s);
}

hipError_t launch_decode_pitched(const uint8_t *grid, uint8_t *img, const PitchedFrames &f, uint32_t k, int interp, const Seeds *seeds, hipStream_t s)
{
    return pitched("launch_decode_pitched", false, grid, img, f, k, interp, Lut256{}, false, seeds, s);
}

hipError_t launch_encode_pitched(const uint8_t *img, uint8_t *grid, const PitchedFrames &f, uint32_t k, int interp, const Lut256 &lut, bool ident,
                                 const Seeds *seeds, hipStream_t s)
{
    return pitched("launch_encode_pitched", true, img, grid, f, k, interp, lut, ident, seeds, s);
}

hipError_t launch_gather_lattice(const uint8_t *src, const Frames &f, uint32_t k, uint8_t *dst, uint32_t sw, uint32_t sh, uint64_t dst_stride,
                                 hipStream_t s)
{
    static const char *name = "launch_gather_lattice";
    const Frames fr = f;
    sim::launch(s, name, [=]() {
        if (!fr.width || !fr.height || !fr.batch || k > 31 || sw != ceil_shift(fr.width, k) || sh != ceil_shift(fr.height, k) ||
            (fr.batch > 1 && dst_stride < (uint64_t)sw * sh))
            sim::die("%s: arguments", name);
        for (uint32_t b = 0; b < fr.batch; ++b) {
            const uint8_t *fp = src + b * fr.frame_stride;
            uint8_t *dp = dst + b * dst_stride;
            sim::dev_check(fp, (size_t)fr.width * fr.height, name);
            sim::dev_check(dp, (size_t)sw * sh, name);
            for (uint64_t y = 0; y < sh; ++y)
                for (uint64_t x = 0; x < sw; ++x) dp[y * sw + x] = fp[(y << k) * fr.width + (x << k)];
        }
    });
    return hipSuccess;
}

bool lattice_pyramid_fits(uint32_t sw, uint32_t sh, size_t batch)
{
    const uint64_t limit = (uint64_t)HGI_KNOB(HGI_LATTICE_MAX, 8192);
    return (uint64_t)sw * sh <= limit && (uint64_t)sw * sh <= 64 * 1024 && batch <= 0x7FFFFFFFull;
}

hipError_t launch_lattice_pyramid(const uint8_t *src, const Frames &f, uint32_t k, uint32_t up, int interp, const Lut256 &lut, bool lut_is_identity,
                                  bool encode, uint8_t *out_q, uint8_t *out_rec, uint32_t sw, uint32_t sh, uint64_t dst_stride, hipStream_t s)
{
    static const char *name = "launch_lattice_pyramid";
    const Frames fr = f;
    const Lut256 l = lut;
    sim::launch(s, name, [=]() {
        if (!fr.width || !fr.height || !fr.batch || k > 31 || up < 1 || up > 31 || sw != ceil_shift(fr.width, k) || sh != ceil_shift(fr.height, k) ||
            (fr.batch > 1 && dst_stride < (uint64_t)sw * sh) || !out_rec || (encode && !out_q) ||
            (interp != kInterpLeftTop && interp != kInterpCrossed))
            sim::die("%s: arguments", name);
        if (!lattice_pyramid_fits(sw, sh, fr.batch)) sim::die("%s: a %u x %u plane does not fit the kernel", name, sw, sh);
        const Table t = encode ? unpack(l, lut_is_identity, name) : Table{};
        const size_t m = (size_t)sw * sh;
        Bytes lat(m), rec(m);
        for (uint32_t b = 0; b < fr.batch; ++b) {
            const uint8_t *fp = src + b * fr.frame_stride;
            sim::dev_check(fp, (size_t)fr.width * fr.height, name);
            for (uint64_t y = 0; y < sh; ++y)
                for (uint64_t x = 0; x < sw; ++x) lat[y * sw + x] = fp[(y << k) * fr.width + (x << k)];
            sim::dev_check(out_rec + b * dst_stride, m, name);
            if (encode) {
                sim::dev_check(out_q + b * dst_stride, m, name);
                ref::encode(lat.data(), out_q + b * dst_stride, rec.data(), sw, sh, up, interp, t.v);
                memcpy(out_rec + b * dst_stride, rec.data(), m);
            } else {
                ref::decode(lat.data(), out_rec + b * dst_stride, sw, sh, up, interp);
            }
        }
    });
    return hipSuccess;
}

// ---- level-wise path and harness launches ----------------------------------------------------------------------------

namespace {

void check_frames(const char *name, const Frames &f)
{
    if (!f.width || !f.height || !f.batch || (f.batch > 1 && f.frame_stride < (uint64_t)f.width * f.height)) sim::die("%s: frames", name);
}

}  // namespace

hipError_t launch_seed(const uint8_t *src, uint8_t *dst, const Frames &f, uint32_t levels, hipStream_t s)
{
    static const char *name = "launch_seed";
    const Frames fr = f;
    sim::launch(s, name, [=]() {
        check_frames(name, fr);
        if (levels > 31) sim::die("%s: levels", name);
        for (uint32_t b = 0; b < fr.batch; ++b) {
            sim::dev_check(src + b * fr.frame_stride, (size_t)fr.width * fr.height, name);
            sim::dev_check(dst + b * fr.frame_stride, (size_t)fr.width * fr.height, name);
            ref::seed(src + b * fr.frame_stride, dst + b * fr.frame_stride, fr.width, fr.height, levels);
        }
    });
    return hipSuccess;
}

hipError_t launch_decode_level(const uint8_t *grid, uint8_t *img, const Frames &f, uint32_t log2sub, int interp, hipStream_t s)
{
    static const char *name = "launch_decode_level";
    const Frames fr = f;
    sim::launch(s, name, [=]() {
        check_frames(name, fr);
        if (log2sub > 30 || (interp != kInterpLeftTop && interp != kInterpCrossed)) sim::die("%s: arguments", name);
        for (uint32_t b = 0; b < fr.batch; ++b) {
            sim::dev_check(grid + b * fr.frame_stride, (size_t)fr.width * fr.height, name);
            sim::dev_check(img + b * fr.frame_stride, (size_t)fr.width * fr.height, name);
            ref::decode_level(grid + b * fr.frame_stride, img + b * fr.frame_stride, fr.width, fr.height, log2sub, interp);
        }
    });
    return hipSuccess;
}

hipError_t launch_encode_level(uint8_t *rec, uint8_t *grid, const Frames &f, uint32_t log2sub, int interp, const Lut256 &lut, hipStream_t s)
{
    static const char *name = "launch_encode_level";
    const Frames fr = f;
    const Lut256 l = lut;
    sim::launch(s, name, [=]() {
        check_frames(name, fr);
        if (log2sub > 30 || (interp != kInterpLeftTop && interp != kInterpCrossed)) sim::die("%s: arguments", name);
        Table t;
        memcpy(t.v, l.w, 256);
        for (uint32_t b = 0; b < fr.batch; ++b) {
            sim::dev_check(rec + b * fr.frame_stride, (size_t)fr.width * fr.height, name);
            sim::dev_check(grid + b * fr.frame_stride, (size_t)fr.width * fr.height, name);
            ref::encode_level(rec + b * fr.frame_stride, grid + b * fr.frame_stride, fr.width, fr.height, log2sub, interp, t.v);
        }
    });
    return hipSuccess;
}

hipError_t launch_synth(int kind, uint64_t seed, uint64_t first_frame, uint8_t *out, const Frames &f, hipStream_t s)
{
    static const char *name = "launch_synth";
    const Frames fr = f;
    sim::launch(s, name, [=]() {
        check_frames(name, fr);
        for (uint32_t b = 0; b < fr.batch; ++b) {
            sim::dev_check(out + b * fr.frame_stride, (size_t)fr.width * fr.height, name);
            if (hgi_oracle_synth(kind, seed, first_frame + b, fr.width, fr.height, out + b * fr.frame_stride)) sim::die("%s: kind %d", name, kind);
        }
    });
    return hipSuccess;
}

hipError_t launch_copy(const uint8_t *src, uint8_t *dst, size_t n, hipStream_t s)
{
    sim::launch(s, "launch_copy", [=]() {
        sim::dev_check(src, n, "launch_copy");
        sim::dev_check(dst, n, "launch_copy");
        memmove(dst, src, n);
    });
    return hipSuccess;
}

hipError_t launch_histogram(const uint8_t *src, const Frames &f, unsigned long long *hist, hipStream_t s)
{
    static const char *name = "launch_histogram";
    const Frames fr = f;
    sim::launch(s, name, [=]() {
        if (!fr.batch) sim::die("%s: frames", name);
        const size_t n = (size_t)fr.width * fr.height;
        sim::dev_check(hist, 256 * sizeof(unsigned long long) * fr.batch, name);
        memset(hist, 0, 256 * sizeof(unsigned long long) * fr.batch);
        for (uint32_t b = 0; b < fr.batch && n; ++b) {
            sim::dev_check(src + b * fr.frame_stride, n, name);
            for (size_t i = 0; i < n; ++i) ++hist[256 * (size_t)b + src[b * fr.frame_stride + i]];
        }
    });
    return hipSuccess;
}

// out[3 * f + 0] = sum of squared differences, + 1 = largest absolute difference, + 2 = differing pixels (include/hgi.h)
hipError_t launch_diff_stats(const uint8_t *a, const uint8_t *b, const Frames &f, unsigned long long *out, hipStream_t s)
{
    static const char *name = "launch_diff_stats";
    const Frames fr = f;
    sim::launch(s, name, [=]() {
        if (!fr.batch) sim::die("%s: frames", name);
        const size_t n = (size_t)fr.width * fr.height;
        sim::dev_check(out, 3 * sizeof(unsigned long long) * fr.batch, name);
        memset(out, 0, 3 * sizeof(unsigned long long) * fr.batch);
        for (uint32_t fi = 0; fi < fr.batch && n; ++fi) {
            const uint8_t *pa = a + fi * fr.frame_stride, *pb = b + fi * fr.frame_stride;
            sim::dev_check(pa, n, name);
            sim::dev_check(pb, n, name);
            for (size_t i = 0; i < n; ++i) {
                const unsigned long long dd = pa[i] > pb[i] ? pa[i] - pb[i] : pb[i] - pa[i];
                out[3 * (size_t)fi] += dd * dd;
                if (dd > out[3 * (size_t)fi + 1]) out[3 * (size_t)fi + 1] = dd;
                out[3 * (size_t)fi + 2] += dd != 0;
            }
        }
    });
    return hipSuccess;
}

}  // namespace hgi
