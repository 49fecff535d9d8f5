// C ABI of libhgi_mviews.so (include/hgi_mviews.h): mapped view lists.  The plan entry -- pure host code, no HIP call: the rules
// of a list and the blob (hgi_mviews_plan.h) -- and the launch entry, one launch (hgi_fused_mviews_dec.hip).  Stateless: no ctx,
// no scratch, no environment.  Every argument rule is decided before the first HIP call, the HGI_EINVAL rules before the
// HGI_EUNSUPPORTED ones.
#include <hip/hip_runtime.h>
#include <string.h>

#include "../../include/hgi_mviews.h"
#include "../companion/hgi_entry.h"
#include "hgi_mviews_kernels.h"

using namespace hgi;

namespace {

// The argument rules of the launch entry, in the header's order.  Returns HGI_OK with *k / *up set when the launch may go ahead.
hgi_status judge_launch(const void *d_plan, const hgi_mviews_info *info, uint32_t levels, hgi_interp interp, const void *d_table, uint32_t *k,
                        uint32_t *up)
{
    // ---- HGI_EINVAL ----
    if (!info) return fail(HGI_EINVAL, "info is NULL");
    if (!mviews_info_consistent(*info))
        return fail(HGI_EINVAL, "info is not what hgi_mviews_plan wrote (magic, elem_size, sizes and offsets against the count %u, block count, output interval)",
                    info->count);
    if (!d_plan) return fail(HGI_EINVAL, "d_plan is NULL");
    if (reinterpret_cast<uintptr_t>(d_plan) % 16 != 0) return fail(HGI_EINVAL, "d_plan is not 16-byte aligned");
    if (!d_table) return fail(HGI_EINVAL, "d_table is NULL");
    const Interval ti = table_interval(reinterpret_cast<uintptr_t>(d_table), 256u * (uint64_t)info->elem_size);
    const Interval oi = {info->dst_lo, info->dst_hi};
    if (meet(ti, oi))
        return fail(HGI_EINVAL, "the table's %u bytes lie inside the byte interval of the outputs: they must not alias (tested conservatively, on the interval that holds every output span)",
                    256u * info->elem_size);
    if (levels > 31) return fail(HGI_EINVAL, "levels %u out of range 0..=31", levels);
    if (interp != HGI_INTERP_LEFTTOP && interp != HGI_INTERP_CROSSED)
        return fail(HGI_EINVAL, "interpolator %d unknown (0 = LeftTop, 1 = Crossed)", (int)interp);
    // ---- HGI_EUNSUPPORTED ----
    if (levels == 0 || levels > 8)
        return fail(HGI_EUNSUPPORTED, "levels %u: one launch serves 1..=8 levels (compose one mapped decode per view)", levels);
    split_levels(levels, k, up);
    return HGI_OK;
}

bool empty_plan(const hgi_mviews_info *info) { return info && info->magic == HGI_MVIEWS_MAGIC && info->count == 0 && mviews_info_consistent(*info); }

}  // namespace

extern "C" {

size_t hgi_mviews_plan_bytes(size_t n) { return n > (SIZE_MAX - 64) / 96 ? SIZE_MAX : (size_t)views_blob_bytes(n); }

hgi_status hgi_mviews_plan(const hgi_mview_pair *views, size_t n, uint32_t elem_size, void *h_plan, size_t plan_bytes, hgi_mviews_info *info)
{
    // an empty list succeeds: a plan of no frame, which the launch accepts and does nothing for
    if (n == 0) {
        if (info) {
            memset(info, 0, sizeof(*info));
            mviews_plan(nullptr, 0, elem_size == 2 || elem_size == 4 ? elem_size : 0, nullptr, info);
        }
        return HGI_OK;
    }
    // ---- HGI_EINVAL ----
    if (!views || !h_plan || !info) {
        if (info) memset(info, 0, sizeof(*info));
        return fail(HGI_EINVAL, "NULL argument (views, h_plan or info)");
    }
    memset(info, 0, sizeof(*info));
    if (plan_bytes < hgi_mviews_plan_bytes(n))
        return fail(HGI_EINVAL, "plan_bytes %zu < hgi_mviews_plan_bytes(%zu) = %zu", plan_bytes, n, hgi_mviews_plan_bytes(n));
    if (elem_size != 2 && elem_size != 4) return fail(HGI_EINVAL, "elem_size %u: table elements are 2 or 4 bytes", elem_size);
    const MViewsJudged j = mviews_plan(views, n, elem_size, h_plan, info);
    const hgi_mview_pair &v = views[j.verdict == kMViewsOk || j.verdict == kMViewsTiles ? 0 : j.a];
    switch (j.verdict) {
    case kMViewsOk: return HGI_OK;
    case kMViewsNullEntry: return fail(HGI_EINVAL, "view %zu: NULL %s", j.a, !v.src ? "src" : "dst");
    case kMViewsSrcPitch: return fail(HGI_EINVAL, "view %zu: source pitch %llu < width %u", j.a, (unsigned long long)v.src_pitch, v.width);
    case kMViewsDstAlign: return fail(HGI_EINVAL, "view %zu: dst is not aligned to elem_size %u", j.a, elem_size);
    case kMViewsDstPitchAlign:
        return fail(HGI_EINVAL, "view %zu: destination pitch %llu is not a multiple of elem_size %u", j.a, (unsigned long long)v.dst_pitch, elem_size);
    case kMViewsDstPitch:
        return fail(HGI_EINVAL, "view %zu: destination pitch %llu < width %u * elem_size %u", j.a, (unsigned long long)v.dst_pitch, v.width, elem_size);
    case kMViewsTiles: return fail(HGI_EINVAL, "more tiles than a launch holds");
    case kMViewsOutOut:
        return fail(HGI_EINVAL, j.mixed_pitch ? "the outputs of views %zu and %zu: their byte spans meet and their pitches differ (not judged: refused)"
                                              : "the outputs of views %zu and %zu share bytes: outputs must be disjoint rectangles",
                    j.a, j.b);
    case kMViewsOutIn:
        return fail(HGI_EINVAL, j.mixed_pitch ? "the output of view %zu and the input of view %zu: their byte spans meet and their pitches differ (not judged: refused)"
                                              : "the output of view %zu shares bytes with the input of view %zu: no output may meet an input",
                    j.a, j.b);
    // ---- HGI_EUNSUPPORTED ----
    case kMViewsFits32:
        return fail(HGI_EUNSUPPORTED, "view %zu: its offsets do not fit the 32-bit buffer path (byte pitch and height too large; compose one mapped decode per view)", j.a);
    case kMViewsTail:
        return fail(HGI_EUNSUPPORTED, "view %zu: width %u is not a multiple of 4 and the three tail bytes behind its source span leave its 4-KiB page (compose one mapped decode per view)", j.a, v.width);
    }
    return fail(HGI_EINVAL, "unknown verdict");
}

hgi_status hgi_mviews_decode_dev(void *hip_stream, const void *d_plan, const hgi_mviews_info *info, uint32_t levels, hgi_interp interp,
                                 const void *d_table)
{
    // a plan of no frame succeeds and does nothing, whatever the other arguments
    if (empty_plan(info)) return HGI_OK;
    uint32_t k, up;
    const hgi_status st = judge_launch(d_plan, info, levels, interp, d_table, &k, &up);
    if (st != HGI_OK) return st;
    const hipError_t e = launch_mviews_decode(mview_args(d_plan, *info), info->max_width, d_table, info->elem_size, k, up, (int)interp,
                                              static_cast<hipStream_t>(hip_stream));
    if (e != hipSuccess) return fail(HGI_EDEVICE, "HIP error %d (%s) in the mapped view-list launch", (int)e, hipGetErrorString(e));
    return HGI_OK;
}

const char *hgi_mviews_last_error(void) { return g_err; }

const char *hgi_mviews_version(void) { return "hgi_mviews 1.0 (HIP, gfx950: mapped view lists, grids to float frames with a pitch of their own in one launch)"; }

}  // extern "C"
