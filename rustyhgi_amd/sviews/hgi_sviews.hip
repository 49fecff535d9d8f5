// C ABI of libhgi_sviews.so (include/hgi_sviews.h): scaled view lists.  The plan entry -- pure host code, no HIP call: the rules
// of a list and the blob (hgi_sviews_plan.h) -- and the launch entry: the judgement -- one plain C++ function of that header that
// returns a status and a message -- and then one launch (hgi_fused_sviews_dec.hip).  Stateless: no ctx, no scratch, no
// environment.  Every argument rule is decided before the first HIP call, the HGI_EINVAL rules before the HGI_EUNSUPPORTED ones.
#include <hip/hip_runtime.h>
#include <string.h>

#include "../../include/hgi_sviews.h"
#include "../companion/hgi_entry.h"
#include "hgi_sviews_kernels.h"

using namespace hgi;

extern "C" {

size_t hgi_sviews_plan_bytes(size_t n) { return n > (SIZE_MAX - 64) / 96 ? SIZE_MAX : (size_t)views_blob_bytes(n); }

hgi_status hgi_sviews_plan(const hgi_sview_pair *views, size_t n, uint32_t shift, void *h_plan, size_t plan_bytes, hgi_sviews_info *info)
{
    // an empty list succeeds: a plan of no grid, which the launch accepts and does nothing for
    if (n == 0) {
        if (info) {
            memset(info, 0, sizeof(*info));
            sviews_plan(nullptr, 0, shift <= 31 ? shift : 0, nullptr, info);
        }
        return HGI_OK;
    }
    // ---- HGI_EINVAL ----
    if (!views || !h_plan || !info) {
        if (info) memset(info, 0, sizeof(*info));
        return fail(HGI_EINVAL, "NULL argument (views, h_plan or info)");
    }
    memset(info, 0, sizeof(*info));
    if (plan_bytes < hgi_sviews_plan_bytes(n))
        return fail(HGI_EINVAL, "plan_bytes %zu < hgi_sviews_plan_bytes(%zu) = %zu", plan_bytes, n, hgi_sviews_plan_bytes(n));
    if (shift > 31) return fail(HGI_EINVAL, "shift %u out of range 0..=31", shift);
    const SViewsJudged j = sviews_plan(views, n, shift, h_plan, info);
    const hgi_sview_pair &v = views[j.verdict == kSViewsOk || j.verdict == kSViewsTiles || j.verdict == kSViewsShiftZero ? 0 : j.a];
    switch (j.verdict) {
    case kSViewsOk: return HGI_OK;
    case kSViewsNullEntry: return fail(HGI_EINVAL, "view %zu: NULL %s", j.a, !v.src ? "src" : "dst");
    case kSViewsSrcPitch: return fail(HGI_EINVAL, "view %zu: source pitch %llu < width %u", j.a, (unsigned long long)v.src_pitch, v.width);
    case kSViewsDstPitch:
        return fail(HGI_EINVAL, "view %zu: destination pitch %llu < scaled width %u", j.a, (unsigned long long)v.dst_pitch, sview_dim(v.width, shift));
    case kSViewsTiles: return fail(HGI_EINVAL, "more tiles than a launch holds");
    case kSViewsOutOut:
        return fail(HGI_EINVAL, j.mixed_pitch ? "the outputs of views %zu and %zu: their byte spans meet and their pitches differ (not judged: refused)"
                                              : "the outputs of views %zu and %zu share bytes: outputs must be disjoint rectangles",
                    j.a, j.b);
    case kSViewsOutIn:
        return fail(HGI_EINVAL, j.mixed_pitch ? "the output of view %zu and the grid of view %zu: their byte spans meet and their pitches differ (not judged: refused)"
                                              : "the output of view %zu shares bytes with the grid of view %zu: no output may meet an input",
                    j.a, j.b);
    // ---- HGI_EUNSUPPORTED ----
    case kSViewsShiftZero: return fail(HGI_EUNSUPPORTED, "shift 0 is full resolution: that is hgi_views_plan's list");
    case kSViewsRead32:
        return fail(HGI_EUNSUPPORTED, "view %zu: its grid's offsets do not fit the 32-bit buffer path (span, or source pitch << shift and height, too large; compose one scaled decode per view)", j.a);
    case kSViewsWrite32:
        return fail(HGI_EUNSUPPORTED, "view %zu: its output's offsets do not fit the 32-bit buffer path (destination pitch and scaled height too large; compose one scaled decode per view)", j.a);
    }
    return fail(HGI_EINVAL, "unknown verdict");
}

hgi_status hgi_sviews_decode_dev(void *hip_stream, const void *d_plan, const hgi_sviews_info *info, uint32_t levels, hgi_interp interp)
{
    const SViewsLaunchJudged j = sviews_judge(d_plan, info, levels, interp);
    // a plan of no grid succeeds and does nothing, whatever the other arguments
    if (j.verdict == kSViewsEmpty) return HGI_OK;
    if (j.status == HGI_EINVAL) return fail(HGI_EINVAL, "%s", j.text);
    if (j.status != HGI_OK) return fail(HGI_EUNSUPPORTED, "%s", j.text);
    const hipError_t e = launch_sviews_decode(sview_args(d_plan, *info), info->max_width, info->shift, j.k, j.up, (int)interp,
                                              static_cast<hipStream_t>(hip_stream));
    if (e != hipSuccess) return fail(HGI_EDEVICE, "HIP error %d (%s) in the scaled view-list launch", (int)e, hipGetErrorString(e));
    return HGI_OK;
}

const char *hgi_sviews_last_error(void) { return g_err; }

const char *hgi_sviews_version(void) { return "hgi_sviews 1.0 (HIP, gfx950: scaled view lists, grids with a pitch of their own at 1/2^s resolution in one launch)"; }

}  // extern "C"
