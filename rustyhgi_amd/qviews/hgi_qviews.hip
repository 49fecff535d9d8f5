// C ABI of libhgi_qviews.so (include/hgi_qviews.h): requantize view lists.  The launch entry: the judgement -- pure host code, no
// HIP call: every rule of the call, in one function that returns a status and a message (hgi_qviews_plan.h) -- and then one
// launch (hgi_fused_qviews.hip).  The plan of a list is hgi_views_plan's: this library has no plan entry.  Stateless: no ctx, no
// scratch, no environment.  Every argument rule is decided before the first HIP call, the HGI_EINVAL rules before the
// HGI_EUNSUPPORTED ones.
#include <hip/hip_runtime.h>
#include <string.h>

#include "../../include/hgi_qviews.h"
#include "../companion/hgi_entry.h"
#include "hgi_qviews_kernels.h"

using namespace hgi;

extern "C" {

hgi_status hgi_qviews_requant_dev(void *hip_stream, const void *d_plan, const hgi_views_info *info, uint32_t levels, hgi_interp interp,
                                  const uint8_t lut[256])
{
    const QViewsJudged j = qviews_judge(d_plan, info, levels, interp, lut);
    // a plan of no frame succeeds and does nothing, whatever the other arguments
    if (j.verdict == kQViewsEmpty) return HGI_OK;
    if (j.status == HGI_EINVAL) return fail(HGI_EINVAL, "%s", j.text);
    if (j.status != HGI_OK) return fail(HGI_EUNSUPPORTED, "%s", j.text);
    Lut256 l;
    memcpy(l.w, lut, 256);
    const hipError_t e = launch_qviews_requant(view_args(d_plan, *info), j.k, j.up, (int)interp, l, static_cast<hipStream_t>(hip_stream));
    if (e != hipSuccess) return fail(HGI_EDEVICE, "HIP error %d (%s) in the requantize view-list launch", (int)e, hipGetErrorString(e));
    return HGI_OK;
}

const char *hgi_qviews_last_error(void) { return g_err; }

const char *hgi_qviews_version(void) { return "hgi_qviews 1.0 (HIP, gfx950: requantize view lists, grids with a pitch of their own re-coded in one launch)"; }

}  // extern "C"
