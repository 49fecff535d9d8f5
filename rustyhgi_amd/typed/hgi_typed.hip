// C ABI of libhgi_typed.so (include/hgi_typed.h): typed encode.  Argument rules, the two-sided plan (hgi_typed_plan.h) and the
// one launch (hgi_fused_typed_enc.hip).  Stateless: no ctx, no scratch, no environment.  Every argument rule is decided before
// the first HIP call, the HGI_EINVAL rules before the HGI_EUNSUPPORTED ones.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include "../../include/hgi_typed.h"
#include "../companion/hgi_entry.h"
#include "hgi_typed_kernels.h"

using namespace hgi;

extern "C" {

hgi_status hgi_typed_encode_dev(void *hip_stream, const void *d_img, size_t img_pitch, uint32_t elem_size, uint32_t elem_kind,
                                float scale, float bias, uint32_t width, uint32_t height, uint32_t levels, hgi_interp interp,
                                const uint8_t lut[256], void *d_grid, size_t grid_pitch, size_t batch, size_t img_frame_stride,
                                size_t grid_frame_stride)
{
    typedef unsigned __int128 u128;
    // an empty call succeeds and does nothing, whatever its other arguments
    if (width == 0 || height == 0 || batch == 0) return HGI_OK;
    // ---- HGI_EINVAL ----
    if (!lut) return fail(HGI_EINVAL, "lut is NULL");
    if (!d_img || !d_grid) return fail(HGI_EINVAL, "NULL buffer");
    if (levels > 31) return fail(HGI_EINVAL, "levels %u out of range 0..=31", levels);
    if (elem_size != 2 && elem_size != 4) return fail(HGI_EINVAL, "elem_size %u: image elements are 2 or 4 bytes", elem_size);
    if (elem_kind > 1) return fail(HGI_EINVAL, "elem_kind %u: 0 = IEEE (float16 / float32), 1 = bfloat16", elem_kind);
    if (elem_kind == 1 && elem_size != 2) return fail(HGI_EINVAL, "elem_kind 1 (bfloat16) goes with elem_size 2, not %u", elem_size);
    if (!isfinite(scale) || !isfinite(bias)) return fail(HGI_EINVAL, "scale and bias must be finite");
    const uint64_t row = (uint64_t)width * elem_size;      // bytes of an image row
    if (reinterpret_cast<uintptr_t>(d_img) % elem_size) return fail(HGI_EINVAL, "d_img is not aligned to elem_size %u", elem_size);
    if (img_pitch % elem_size) return fail(HGI_EINVAL, "image pitch %zu is not a multiple of elem_size %u", img_pitch, elem_size);
    if (batch > 1 && img_frame_stride % elem_size)
        return fail(HGI_EINVAL, "image frame stride %zu is not a multiple of elem_size %u", img_frame_stride, elem_size);
    if (img_pitch < row) return fail(HGI_EINVAL, "image pitch %zu < width %u * elem_size %u", img_pitch, width, elem_size);
    if (grid_pitch < width) return fail(HGI_EINVAL, "grid pitch %zu < width %u", grid_pitch, width);
    if (batch > 0x7fffffffu) return fail(HGI_EINVAL, "batch too large");
    const u128 ispan = (u128)(height - 1) * img_pitch + row, gspan = (u128)(height - 1) * grid_pitch + width;
    if (batch > 1 && (u128)img_frame_stride < ispan)
        return fail(HGI_EINVAL, "image frame stride %zu < (height - 1) * pitch + width * elem_size", img_frame_stride);
    if (batch > 1 && (u128)grid_frame_stride < gspan)
        return fail(HGI_EINVAL, "grid frame stride %zu < (height - 1) * pitch + width", grid_frame_stride);
    // No aliasing, tested conservatively: the byte intervals of the image and the grid must not meet.
    const Interval ii = side_interval(reinterpret_cast<uintptr_t>(d_img), row, height, img_pitch, img_frame_stride, batch);
    const Interval gi = side_interval(reinterpret_cast<uintptr_t>(d_grid), width, height, grid_pitch, grid_frame_stride, batch);
    if (ii.hi - ii.lo > (u128)SIZE_MAX || gi.hi - gi.lo > (u128)SIZE_MAX) return fail(HGI_EINVAL, "frame span too large");
    if (meet(ii, gi)) return fail(HGI_EINVAL, "the grid span overlaps the image span: they must not alias");
    const TypedFrames f = {width, height, (uint32_t)batch, elem_size, (uint64_t)img_pitch, (uint64_t)grid_pitch,
                           (uint64_t)img_frame_stride, (uint64_t)grid_frame_stride};
    const TypedJudged j = typed_plan(reinterpret_cast<uintptr_t>(d_img), f);
    const TypedPlan &tp = j.plan;
    if (!tp.p.ok) return fail(HGI_EINVAL, "more tiles than a launch holds");
    // ---- HGI_EUNSUPPORTED ----
    if (levels == 0 || levels > 8)
        return fail(HGI_EUNSUPPORTED, "levels %u: one launch serves 1..=8 levels (compose conversion + encode)", levels);
    if (!j.fits32)
        return fail(HGI_EUNSUPPORTED, "a side's offsets do not fit the 32-bit buffer path (pitch and height too large; compose conversion + encode)");
    if (interp != HGI_INTERP_LEFTTOP && interp != HGI_INTERP_CROSSED)
        return fail(HGI_EUNSUPPORTED, "interpolator %d not implemented (0 = LeftTop, 1 = Crossed)", (int)interp);
    if (!j.tail_ok)
        return fail(HGI_EUNSUPPORTED, "2-byte elements, width %u is odd and the two tail bytes behind the last image frame's span leave its 4-KiB page (compose conversion + encode)", width);
    if (!tp.p.fast) return fail(HGI_EUNSUPPORTED, "the call does not take the buffer path (compose conversion + encode)");
    Lut256 l;
    memcpy(l.w, lut, 256);
    bool ident = true;
    for (int i = 0; i < 256; ++i) ident = ident && lut[i] == i;
    uint32_t k, up;
    split_levels(levels, &k, &up);
    const hipError_t e = launch_encode_typed(d_img, static_cast<uint8_t *>(d_grid), tp, elem_size, elem_kind == 1, scale, bias, k, up,
                                             (int)interp, l, ident, static_cast<hipStream_t>(hip_stream));
    if (e != hipSuccess) return fail(HGI_EDEVICE, "HIP error %d (%s) in the typed encode launch", (int)e, hipGetErrorString(e));
    return HGI_OK;
}

const char *hgi_typed_last_error(void) { return g_err; }

const char *hgi_typed_version(void) { return "hgi_typed 1.0 (HIP, gfx950: typed encode)"; }

}  // extern "C"
