// C ABI of libhgi_rviews.so (include/hgi_rviews.h): recon view lists.  The plan entry -- pure host code, no HIP call: the rules
// of a list and the blob (hgi_rviews_plan.h) -- and the launch entry: the judgement -- one plain C++ function of that header that
// returns a status and a message -- and then one launch (hgi_fused_rviews_enc.hip).  Stateless: no ctx, no scratch, no
// environment.  Every argument rule is decided before the first HIP call, the HGI_EINVAL rules before the HGI_EUNSUPPORTED ones.
#include <hip/hip_runtime.h>
#include <string.h>

#include "../../include/hgi_rviews.h"
#include "../companion/hgi_entry.h"
#include "hgi_rviews_kernels.h"

using namespace hgi;

extern "C" {

size_t hgi_rviews_plan_bytes(size_t n) { return n > (SIZE_MAX - 64) / 112 ? SIZE_MAX : (size_t)rviews_blob_bytes(n); }

hgi_status hgi_rviews_plan(const hgi_rview_triple *triples, size_t n, void *h_plan, size_t plan_bytes, hgi_rviews_info *info)
{
    if (info) memset(info, 0, sizeof(*info));
    // an empty list succeeds: a plan of no frame, which the launch accepts and does nothing for
    if (n == 0) {
        if (info) rviews_plan(nullptr, 0, nullptr, info);
        return HGI_OK;
    }
    // ---- HGI_EINVAL ----
    if (!triples || !h_plan || !info) return fail(HGI_EINVAL, "NULL argument (triples, h_plan or info)");
    if (plan_bytes < hgi_rviews_plan_bytes(n))
        return fail(HGI_EINVAL, "plan_bytes %zu < hgi_rviews_plan_bytes(%zu) = %zu", plan_bytes, n, hgi_rviews_plan_bytes(n));
    const RViewsJudged j = rviews_plan(triples, n, h_plan, info);
    const hgi_rview_triple &t = triples[j.verdict == kRViewsOk || j.verdict == kRViewsTiles ? 0 : j.a];
    static const char *const side[2] = {"grid", "reconstruction"};
    switch (j.verdict) {
    case kRViewsOk: return HGI_OK;
    case kRViewsNullEntry: return fail(HGI_EINVAL, "view %zu: NULL %s", j.a, !t.src ? "src" : !t.grid ? "grid" : "recon");
    case kRViewsSrcPitch: return fail(HGI_EINVAL, "view %zu: source pitch %llu < width %u", j.a, (unsigned long long)t.src_pitch, t.width);
    case kRViewsGridPitch: return fail(HGI_EINVAL, "view %zu: grid pitch %llu < width %u", j.a, (unsigned long long)t.grid_pitch, t.width);
    case kRViewsReconPitch:
        return fail(HGI_EINVAL, "view %zu: reconstruction pitch %llu < width %u", j.a, (unsigned long long)t.recon_pitch, t.width);
    case kRViewsTiles: return fail(HGI_EINVAL, "more tiles than a launch holds");
    case kRViewsOutOut:
        return fail(HGI_EINVAL, j.mixed_pitch ? "the %s of view %zu and the %s of view %zu: their byte spans meet and their pitches differ (not judged: refused)"
                                              : "the %s of view %zu and the %s of view %zu share bytes: outputs must be disjoint rectangles",
                    side[j.side_a], j.a, side[j.side_b], j.b);
    case kRViewsOutIn:
        return fail(HGI_EINVAL, j.mixed_pitch ? "the %s of view %zu and the input of view %zu: their byte spans meet and their pitches differ (not judged: refused)"
                                              : "the %s of view %zu shares bytes with the input of view %zu: no output may meet an input (in place is refused: a tile's halo reads its neighbours' originals)",
                    side[j.side_a], j.a, j.b);
    // ---- HGI_EUNSUPPORTED ----
    case kRViewsFits32:
        return fail(HGI_EUNSUPPORTED, "view %zu: its offsets do not fit the 32-bit buffer path (the largest of its three pitches and its height are too large; compose one encode with reconstruction per view)", j.a);
    case kRViewsTail:
        return fail(HGI_EUNSUPPORTED, "view %zu: width %u is not a multiple of 4 and the three tail bytes behind its source span leave its 4-KiB page (compose one encode with reconstruction per view)", j.a, t.width);
    }
    return fail(HGI_EINVAL, "unknown verdict");
}

hgi_status hgi_rviews_encode_dev(void *hip_stream, const void *d_plan, const hgi_rviews_info *info, uint32_t levels, hgi_interp interp,
                                 const uint8_t *lut)
{
    const RViewsLaunchJudged j = rviews_judge(d_plan, info, levels, interp, lut);
    // a plan of no frame succeeds and does nothing, whatever the other arguments
    if (j.verdict == kRViewsEmpty) return HGI_OK;
    if (j.status == HGI_EINVAL) return fail(HGI_EINVAL, "%s", j.text);
    if (j.status != HGI_OK) return fail(HGI_EUNSUPPORTED, "%s", j.text);
    Lut256 l;
    memcpy(l.w, lut, 256);
    const hipError_t e = launch_rviews_encode(rview_args(d_plan, *info), j.k, j.up, (int)interp, l, j.ident, static_cast<hipStream_t>(hip_stream));
    if (e != hipSuccess) return fail(HGI_EDEVICE, "HIP error %d (%s) in the recon view-list launch", (int)e, hipGetErrorString(e));
    return HGI_OK;
}

const char *hgi_rviews_last_error(void) { return g_err; }

const char *hgi_rviews_version(void) { return "hgi_rviews 1.0 (HIP, gfx950: recon view lists, grids and reconstructions of frames with pitches of their own in one launch)"; }

}  // extern "C"
