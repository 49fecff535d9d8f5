// C ABI of libhgi_requant.so (include/hgi_requant.h): requantize.  Argument rules, the two-sided plan (hgi_requant_plan.h) and
// the one launch (hgi_fused_requant.hip).  Stateless: no ctx, no scratch, no environment.  Every argument rule is decided before
// the first HIP call, the HGI_EINVAL rules before the HGI_EUNSUPPORTED ones.
#include <hip/hip_runtime.h>
#include <string.h>

#include "../../include/hgi_requant.h"
#include "../companion/hgi_entry.h"
#include "hgi_requant_kernels.h"

using namespace hgi;

extern "C" {

hgi_status hgi_requant_dev(void *hip_stream, const void *d_src, size_t src_pitch, uint32_t width, uint32_t height, uint32_t levels,
                           hgi_interp interp, const uint8_t lut[256], void *d_dst, size_t dst_pitch, size_t batch,
                           size_t src_frame_stride, size_t dst_frame_stride)
{
    typedef unsigned __int128 u128;
    // an empty call succeeds and does nothing, whatever its other arguments
    if (width == 0 || height == 0 || batch == 0) return HGI_OK;
    // ---- HGI_EINVAL ----
    if (!lut) return fail(HGI_EINVAL, "lut is NULL");
    if (!d_src || !d_dst) return fail(HGI_EINVAL, "NULL buffer");
    if (levels > 31) return fail(HGI_EINVAL, "levels %u out of range 0..=31", levels);
    if (src_pitch < width) return fail(HGI_EINVAL, "source pitch %zu < width %u", src_pitch, width);
    if (dst_pitch < width) return fail(HGI_EINVAL, "destination pitch %zu < width %u", dst_pitch, width);
    if (batch > 0x7fffffffu) return fail(HGI_EINVAL, "batch too large");
    const u128 sspan = (u128)(height - 1) * src_pitch + width, dspan = (u128)(height - 1) * dst_pitch + width;
    if (batch > 1 && (u128)src_frame_stride < sspan)
        return fail(HGI_EINVAL, "source frame stride %zu < (height - 1) * pitch + width", src_frame_stride);
    if (batch > 1 && (u128)dst_frame_stride < dspan)
        return fail(HGI_EINVAL, "destination frame stride %zu < (height - 1) * pitch + width", dst_frame_stride);
    // No aliasing, tested conservatively: the byte intervals the two sides span must not meet.
    const Interval si = side_interval(reinterpret_cast<uintptr_t>(d_src), width, height, src_pitch, src_frame_stride, batch);
    const Interval di = side_interval(reinterpret_cast<uintptr_t>(d_dst), width, height, dst_pitch, dst_frame_stride, batch);
    if (si.hi - si.lo > (u128)SIZE_MAX || di.hi - di.lo > (u128)SIZE_MAX) return fail(HGI_EINVAL, "frame span too large");
    if (meet(si, di))
        return fail(HGI_EINVAL, d_dst == d_src ? "in-place (d_dst == d_src) is refused: a tile's halo reads its neighbours' source residuals (the spans overlap)"
                                               : "the destination span overlaps the source span: they must not alias");
    const RequantFrames f = {width, height, (uint32_t)batch, (uint64_t)src_pitch, (uint64_t)dst_pitch, (uint64_t)src_frame_stride,
                             (uint64_t)dst_frame_stride};
    const RequantJudged j = requant_plan(reinterpret_cast<uintptr_t>(d_src), f);
    const PitchedPlan &p = j.plan;
    if (!p.ok) return fail(HGI_EINVAL, "more tiles than a launch holds");
    // ---- HGI_EUNSUPPORTED ----
    if (levels == 0 || levels > 8)
        return fail(HGI_EUNSUPPORTED, "levels %u: one launch serves 1..=8 levels (compose decode + encode)", levels);
    if (interp != HGI_INTERP_LEFTTOP && interp != HGI_INTERP_CROSSED)
        return fail(HGI_EUNSUPPORTED, "interpolator %d not implemented (0 = LeftTop, 1 = Crossed)", (int)interp);
    if (!j.fits32)
        return fail(HGI_EUNSUPPORTED, "a side's offsets do not fit the 32-bit buffer path (pitch and height too large; compose decode + encode)");
    if (!j.tail_ok)
        return fail(HGI_EUNSUPPORTED, "width %u is not a multiple of 4 and the three tail bytes behind the last source frame's span leave its 4-KiB page (compose decode + encode)", width);
    if (!p.fast) return fail(HGI_EUNSUPPORTED, "the call does not take the buffer path (compose decode + encode)");
    bool ident = true;
    for (int i = 0; i < 256; ++i) ident = ident && lut[i] == i;
    if (ident)
        return fail(HGI_EUNSUPPORTED, "the identity table re-codes a grid into itself: copy the source (no kernel is built for it)");
    Lut256 l;
    memcpy(l.w, lut, 256);
    uint32_t k, up;
    split_levels(levels, &k, &up);
    const hipError_t e = launch_requant(static_cast<const uint8_t *>(d_src), static_cast<uint8_t *>(d_dst), p, k, up, (int)interp, l,
                                        static_cast<hipStream_t>(hip_stream));
    if (e != hipSuccess) return fail(HGI_EDEVICE, "HIP error %d (%s) in the requantize launch", (int)e, hipGetErrorString(e));
    return HGI_OK;
}

const char *hgi_requant_last_error(void) { return g_err; }

const char *hgi_requant_version(void) { return "hgi_requant 1.0 (HIP, gfx950: grids re-coded with another quantizer)"; }

}  // extern "C"
