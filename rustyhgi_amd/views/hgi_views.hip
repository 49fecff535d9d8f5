// C ABI of libhgi_views.so (include/hgi_views.h): view lists.  The plan entry -- pure host code, no HIP call: the rules of a
// list and the blob (hgi_views_plan.h) -- and the two launch entries, one launch each (hgi_fused_views_dec.hip,
// hgi_fused_views_enc.hip).  Stateless: no ctx, no scratch, no environment.  Every argument rule is decided before the first HIP
// call, the HGI_EINVAL rules before the HGI_EUNSUPPORTED ones.
#include <hip/hip_runtime.h>
#include <string.h>

#include "../../include/hgi_views.h"
#include "../companion/hgi_entry.h"
#include "hgi_views_kernels.h"

using namespace hgi;

namespace {

// The argument rules the two launch entries share, in the header's order.  `lut`: the encode entry's table (want_lut).
// Returns HGI_OK with *k / *up set when the launch may go ahead.
hgi_status judge_launch(const void *d_plan, const hgi_views_info *info, uint32_t levels, hgi_interp interp, bool want_lut, const uint8_t *lut,
                        uint32_t *k, uint32_t *up)
{
    // ---- HGI_EINVAL ----
    if (!info) return fail(HGI_EINVAL, "info is NULL");
    if (!views_info_consistent(*info))
        return fail(HGI_EINVAL, "info is not what hgi_views_plan wrote (magic, sizes and offsets against the count %u, block count)", info->count);
    if (!d_plan) return fail(HGI_EINVAL, "d_plan is NULL");
    if (reinterpret_cast<uintptr_t>(d_plan) % 16 != 0) return fail(HGI_EINVAL, "d_plan is not 16-byte aligned");
    if (want_lut && !lut) return fail(HGI_EINVAL, "lut is NULL");
    if (levels > 31) return fail(HGI_EINVAL, "levels %u out of range 0..=31", levels);
    if (interp != HGI_INTERP_LEFTTOP && interp != HGI_INTERP_CROSSED)
        return fail(HGI_EINVAL, "interpolator %d unknown (0 = LeftTop, 1 = Crossed)", (int)interp);
    // ---- HGI_EUNSUPPORTED ----
    if (levels == 0 || levels > 8)
        return fail(HGI_EUNSUPPORTED, "levels %u: one launch serves 1..=8 levels (compose one pitched call per view)", levels);
    split_levels(levels, k, up);
    return HGI_OK;
}

bool empty_plan(const hgi_views_info *info) { return info && info->magic == HGI_VIEWS_MAGIC && info->count == 0 && views_info_consistent(*info); }

}  // namespace

extern "C" {

size_t hgi_views_plan_bytes(size_t n) { return n > (SIZE_MAX - 64) / 96 ? SIZE_MAX : (size_t)views_blob_bytes(n); }

hgi_status hgi_views_plan(const hgi_view_pair *views, size_t n, void *h_plan, size_t plan_bytes, hgi_views_info *info)
{
    if (info) memset(info, 0, sizeof(*info));
    // an empty list succeeds: a plan of no frame, which the launches accept and do nothing for
    if (n == 0) {
        if (info) views_plan(nullptr, 0, nullptr, info);
        return HGI_OK;
    }
    // ---- HGI_EINVAL ----
    if (!views || !h_plan || !info) return fail(HGI_EINVAL, "NULL argument (views, h_plan or info)");
    if (plan_bytes < hgi_views_plan_bytes(n))
        return fail(HGI_EINVAL, "plan_bytes %zu < hgi_views_plan_bytes(%zu) = %zu", plan_bytes, n, hgi_views_plan_bytes(n));
    const ViewsJudged j = views_plan(views, n, h_plan, info);
    const hgi_view_pair &v = views[j.verdict == kViewsOk || j.verdict == kViewsTiles ? 0 : j.a];
    switch (j.verdict) {
    case kViewsOk: return HGI_OK;
    case kViewsNullEntry: return fail(HGI_EINVAL, "view %zu: NULL %s", j.a, !v.src ? "src" : "dst");
    case kViewsSrcPitch: return fail(HGI_EINVAL, "view %zu: source pitch %llu < width %u", j.a, (unsigned long long)v.src_pitch, v.width);
    case kViewsDstPitch: return fail(HGI_EINVAL, "view %zu: destination pitch %llu < width %u", j.a, (unsigned long long)v.dst_pitch, v.width);
    case kViewsTiles: return fail(HGI_EINVAL, "more tiles than a launch holds");
    case kViewsOutOut:
        return fail(HGI_EINVAL, j.mixed_pitch ? "the outputs of views %zu and %zu: their byte spans meet and their pitches differ (not judged: refused)"
                                              : "the outputs of views %zu and %zu share bytes: outputs must be disjoint rectangles",
                    j.a, j.b);
    case kViewsOutIn:
        return fail(HGI_EINVAL, j.mixed_pitch ? "the output of view %zu and the input of view %zu: their byte spans meet and their pitches differ (not judged: refused)"
                                              : "the output of view %zu shares bytes with the input of view %zu: no output may meet an input (in place is refused: a tile's halo reads its neighbours' originals)",
                    j.a, j.b);
    // ---- HGI_EUNSUPPORTED ----
    case kViewsFits32:
        return fail(HGI_EUNSUPPORTED, "view %zu: its offsets do not fit the 32-bit buffer path (pitch and height too large; compose one pitched call per view)", j.a);
    case kViewsTail:
        return fail(HGI_EUNSUPPORTED, "view %zu: width %u is not a multiple of 4 and the three tail bytes behind its source span leave its 4-KiB page (compose one pitched call per view)", j.a, v.width);
    }
    return fail(HGI_EINVAL, "unknown verdict");
}

hgi_status hgi_views_encode_dev(void *hip_stream, const void *d_plan, const hgi_views_info *info, uint32_t levels, hgi_interp interp,
                                const uint8_t *lut)
{
    // a plan of no frame succeeds and does nothing, whatever the other arguments
    if (empty_plan(info)) return HGI_OK;
    uint32_t k, up;
    const hgi_status st = judge_launch(d_plan, info, levels, interp, true, lut, &k, &up);
    if (st != HGI_OK) return st;
    bool ident = true;
    for (int i = 0; i < 256; ++i) ident = ident && lut[i] == i;
    Lut256 l;
    memcpy(l.w, lut, 256);
    const hipError_t e = launch_views_encode(view_args(d_plan, *info), k, up, (int)interp, l, ident, static_cast<hipStream_t>(hip_stream));
    if (e != hipSuccess) return fail(HGI_EDEVICE, "HIP error %d (%s) in the view-list encode launch", (int)e, hipGetErrorString(e));
    return HGI_OK;
}

hgi_status hgi_views_decode_dev(void *hip_stream, const void *d_plan, const hgi_views_info *info, uint32_t levels, hgi_interp interp)
{
    if (empty_plan(info)) return HGI_OK;
    uint32_t k, up;
    const hgi_status st = judge_launch(d_plan, info, levels, interp, false, nullptr, &k, &up);
    if (st != HGI_OK) return st;
    const hipError_t e = launch_views_decode(view_args(d_plan, *info), info->max_width, k, up, (int)interp, static_cast<hipStream_t>(hip_stream));
    if (e != hipSuccess) return fail(HGI_EDEVICE, "HIP error %d (%s) in the view-list decode launch", (int)e, hipGetErrorString(e));
    return HGI_OK;
}

const char *hgi_views_last_error(void) { return g_err; }

const char *hgi_views_version(void) { return "hgi_views 1.0 (HIP, gfx950: view lists, frames with a pitch of their own coded in one launch)"; }

}  // extern "C"
