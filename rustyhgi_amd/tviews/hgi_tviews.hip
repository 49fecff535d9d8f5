// C ABI of libhgi_tviews.so (include/hgi_tviews.h): typed view lists.  The plan entry -- pure host code, no HIP call: the rules
// of a list and the blob (hgi_tviews_plan.h) -- and the launch entry, one launch (hgi_fused_tviews_enc.hip).  Stateless: no ctx,
// no scratch, no environment.  Every argument rule is decided before the first HIP call, the HGI_EINVAL rules before the
// HGI_EUNSUPPORTED ones.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include "../../include/hgi_tviews.h"
#include "../companion/hgi_entry.h"
#include "hgi_tviews_kernels.h"

using namespace hgi;

namespace {

// The argument rules of the launch entry, in the header's order.  Returns HGI_OK with *k / *up set when the launch may go ahead.
hgi_status judge_launch(const void *d_plan, const hgi_tviews_info *info, uint32_t elem_kind, float scale, float bias, uint32_t levels,
                        hgi_interp interp, const uint8_t *lut, uint32_t *k, uint32_t *up)
{
    // ---- HGI_EINVAL ----
    if (!info) return fail(HGI_EINVAL, "info is NULL");
    if (!tviews_info_consistent(*info))
        return fail(HGI_EINVAL, "info is not what hgi_tviews_plan wrote (magic, elem_size, sizes and offsets against the count %u, block count)",
                    info->count);
    if (!d_plan) return fail(HGI_EINVAL, "d_plan is NULL");
    if (reinterpret_cast<uintptr_t>(d_plan) % 16 != 0) return fail(HGI_EINVAL, "d_plan is not 16-byte aligned");
    if (!lut) return fail(HGI_EINVAL, "lut is NULL");
    if (elem_kind > 1) return fail(HGI_EINVAL, "elem_kind %u: 0 = IEEE (float16 / float32), 1 = bfloat16", elem_kind);
    if (elem_kind == 1 && info->elem_size != 2)
        return fail(HGI_EINVAL, "elem_kind 1 (bfloat16) goes with a plan made for elem_size 2, not %u", info->elem_size);
    if (!isfinite(scale) || !isfinite(bias)) return fail(HGI_EINVAL, "scale and bias must be finite");
    if (levels > 31) return fail(HGI_EINVAL, "levels %u out of range 0..=31", levels);
    if (interp != HGI_INTERP_LEFTTOP && interp != HGI_INTERP_CROSSED)
        return fail(HGI_EINVAL, "interpolator %d unknown (0 = LeftTop, 1 = Crossed)", (int)interp);
    // ---- HGI_EUNSUPPORTED ----
    if (levels == 0 || levels > 8)
        return fail(HGI_EUNSUPPORTED, "levels %u: one launch serves 1..=8 levels (compose one typed encode per view)", levels);
    split_levels(levels, k, up);
    return HGI_OK;
}

bool empty_plan(const hgi_tviews_info *info) { return info && info->magic == HGI_TVIEWS_MAGIC && info->count == 0 && tviews_info_consistent(*info); }

}  // namespace

extern "C" {

size_t hgi_tviews_plan_bytes(size_t n) { return n > (SIZE_MAX - 64) / 96 ? SIZE_MAX : (size_t)views_blob_bytes(n); }

hgi_status hgi_tviews_plan(const hgi_tview_pair *views, size_t n, uint32_t elem_size, void *h_plan, size_t plan_bytes, hgi_tviews_info *info)
{
    // an empty list succeeds: a plan of no frame, which the launch accepts and does nothing for
    if (n == 0) {
        if (info) {
            memset(info, 0, sizeof(*info));
            tviews_plan(nullptr, 0, elem_size == 2 || elem_size == 4 ? elem_size : 0, nullptr, info);
        }
        return HGI_OK;
    }
    // ---- HGI_EINVAL ----
    if (!views || !h_plan || !info) {
        if (info) memset(info, 0, sizeof(*info));
        return fail(HGI_EINVAL, "NULL argument (views, h_plan or info)");
    }
    memset(info, 0, sizeof(*info));
    if (plan_bytes < hgi_tviews_plan_bytes(n))
        return fail(HGI_EINVAL, "plan_bytes %zu < hgi_tviews_plan_bytes(%zu) = %zu", plan_bytes, n, hgi_tviews_plan_bytes(n));
    if (elem_size != 2 && elem_size != 4) return fail(HGI_EINVAL, "elem_size %u: frame elements are 2 or 4 bytes", elem_size);
    const TViewsJudged j = tviews_plan(views, n, elem_size, h_plan, info);
    const hgi_tview_pair &v = views[j.verdict == kTViewsOk || j.verdict == kTViewsTiles ? 0 : j.a];
    switch (j.verdict) {
    case kTViewsOk: return HGI_OK;
    case kTViewsNullEntry: return fail(HGI_EINVAL, "view %zu: NULL %s", j.a, !v.src ? "src" : "dst");
    case kTViewsSrcAlign: return fail(HGI_EINVAL, "view %zu: src is not aligned to elem_size %u", j.a, elem_size);
    case kTViewsSrcPitchAlign:
        return fail(HGI_EINVAL, "view %zu: source pitch %llu is not a multiple of elem_size %u", j.a, (unsigned long long)v.src_pitch, elem_size);
    case kTViewsSrcPitch:
        return fail(HGI_EINVAL, "view %zu: source pitch %llu < width %u * elem_size %u", j.a, (unsigned long long)v.src_pitch, v.width, elem_size);
    case kTViewsDstPitch: return fail(HGI_EINVAL, "view %zu: destination pitch %llu < width %u", j.a, (unsigned long long)v.dst_pitch, v.width);
    case kTViewsTiles: return fail(HGI_EINVAL, "more tiles than a launch holds");
    case kTViewsOutOut:
        return fail(HGI_EINVAL, j.mixed_pitch ? "the grids of views %zu and %zu: their byte spans meet and their pitches differ (not judged: refused)"
                                              : "the grids of views %zu and %zu share bytes: grids must be disjoint rectangles",
                    j.a, j.b);
    case kTViewsOutIn:
        return fail(HGI_EINVAL, j.mixed_pitch ? "the grid of view %zu and the frame of view %zu: their byte spans meet and their pitches differ (not judged: refused)"
                                              : "the grid of view %zu shares bytes with the frame of view %zu: no grid may meet a frame",
                    j.a, j.b);
    // ---- HGI_EUNSUPPORTED ----
    case kTViewsFits32:
        return fail(HGI_EUNSUPPORTED, "view %zu: its offsets do not fit the 32-bit buffer path (byte pitch and height too large; compose one typed encode per view)", j.a);
    case kTViewsTail:
        return fail(HGI_EUNSUPPORTED, "view %zu: 2-byte elements, width %u is odd and the two tail bytes behind its frame's span leave its 4-KiB page (compose one typed encode per view)", j.a, v.width);
    }
    return fail(HGI_EINVAL, "unknown verdict");
}

hgi_status hgi_tviews_encode_dev(void *hip_stream, const void *d_plan, const hgi_tviews_info *info, uint32_t elem_kind, float scale, float bias,
                                 uint32_t levels, hgi_interp interp, const uint8_t lut[256])
{
    // a plan of no frame succeeds and does nothing, whatever the other arguments
    if (empty_plan(info)) return HGI_OK;
    uint32_t k, up;
    const hgi_status st = judge_launch(d_plan, info, elem_kind, scale, bias, levels, interp, lut, &k, &up);
    if (st != HGI_OK) return st;
    bool ident = true;
    for (int i = 0; i < 256; ++i) ident = ident && lut[i] == i;
    Lut256 l;
    memcpy(l.w, lut, 256);
    const hipError_t e = launch_tviews_encode(tview_args(d_plan, *info), info->elem_size, elem_kind == 1, scale, bias, k, up, (int)interp, l, ident,
                                              static_cast<hipStream_t>(hip_stream));
    if (e != hipSuccess) return fail(HGI_EDEVICE, "HIP error %d (%s) in the typed view-list launch", (int)e, hipGetErrorString(e));
    return HGI_OK;
}

const char *hgi_tviews_last_error(void) { return g_err; }

const char *hgi_tviews_version(void) { return "hgi_tviews 1.0 (HIP, gfx950: typed view lists, float frames with a pitch of their own to grids in one launch)"; }

}  // extern "C"
