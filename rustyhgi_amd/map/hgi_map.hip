// C ABI of libhgi_map.so (include/hgi_map.h): mapped decode.  Argument rules, the two-sided plan (hgi_map_plan.h) and the one
// launch (hgi_fused_map_dec.hip).  Stateless: no ctx, no scratch, no environment.  Every argument rule is decided before the
// first HIP call, the HGI_EINVAL rules before the HGI_EUNSUPPORTED ones.
#include <hip/hip_runtime.h>
#include <string.h>

#include "../../include/hgi_map.h"
#include "../companion/hgi_entry.h"
#include "hgi_map_kernels.h"

using namespace hgi;

extern "C" {

hgi_status hgi_map_decode_dev(void *hip_stream, const void *d_grid, size_t grid_pitch, uint32_t width, uint32_t height,
                              uint32_t levels, hgi_interp interp, const void *d_table, uint32_t elem_size, void *d_out,
                              size_t out_pitch, size_t batch, size_t grid_frame_stride, size_t out_frame_stride)
{
    typedef unsigned __int128 u128;
    // an empty call succeeds and does nothing, whatever its other arguments
    if (width == 0 || height == 0 || batch == 0) return HGI_OK;
    // ---- HGI_EINVAL ----
    if (levels > 31) return fail(HGI_EINVAL, "levels %u out of range 0..=31", levels);
    if (interp != HGI_INTERP_LEFTTOP && interp != HGI_INTERP_CROSSED)
        return fail(HGI_EINVAL, "unknown interpolator %d (0 = LeftTop, 1 = Crossed)", (int)interp);
    if (elem_size != 2 && elem_size != 4) return fail(HGI_EINVAL, "elem_size %u: table elements are 2 or 4 bytes", elem_size);
    if (!d_grid || !d_table || !d_out) return fail(HGI_EINVAL, "NULL buffer");
    const uint64_t row = (uint64_t)width * elem_size;      // bytes of an output row
    if (reinterpret_cast<uintptr_t>(d_out) % elem_size) return fail(HGI_EINVAL, "d_out is not aligned to elem_size %u", elem_size);
    if (out_pitch % elem_size) return fail(HGI_EINVAL, "output pitch %zu is not a multiple of elem_size %u", out_pitch, elem_size);
    if (batch > 1 && out_frame_stride % elem_size)
        return fail(HGI_EINVAL, "output frame stride %zu is not a multiple of elem_size %u", out_frame_stride, elem_size);
    if (grid_pitch < width) return fail(HGI_EINVAL, "grid pitch %zu < width %u", grid_pitch, width);
    if (out_pitch < row) return fail(HGI_EINVAL, "output pitch %zu < width %u * elem_size %u", out_pitch, width, elem_size);
    if (batch > 0x7fffffffu) return fail(HGI_EINVAL, "batch too large");
    const u128 gspan = (u128)(height - 1) * grid_pitch + width, ospan = (u128)(height - 1) * out_pitch + row;
    if (batch > 1 && (u128)grid_frame_stride < gspan)
        return fail(HGI_EINVAL, "grid frame stride %zu < (height - 1) * pitch + width", grid_frame_stride);
    if (batch > 1 && (u128)out_frame_stride < ospan)
        return fail(HGI_EINVAL, "output frame stride %zu < (height - 1) * pitch + width * elem_size", out_frame_stride);
    // No aliasing, tested conservatively: the byte intervals of the grid, the output and the table must not meet.
    const Interval gi = side_interval(reinterpret_cast<uintptr_t>(d_grid), width, height, grid_pitch, grid_frame_stride, batch);
    const Interval oi = side_interval(reinterpret_cast<uintptr_t>(d_out), row, height, out_pitch, out_frame_stride, batch);
    const Interval ti = table_interval(reinterpret_cast<uintptr_t>(d_table), 256u * (uint64_t)elem_size);
    if (gi.hi - gi.lo > (u128)SIZE_MAX || oi.hi - oi.lo > (u128)SIZE_MAX) return fail(HGI_EINVAL, "frame span too large");
    if (meet(ti, oi)) return fail(HGI_EINVAL, "the table overlaps the output span: they must not alias");
    if (meet(ti, gi)) return fail(HGI_EINVAL, "the table overlaps the grid span: they must not alias");
    if (meet(gi, oi)) return fail(HGI_EINVAL, "the output span overlaps the grid span: they must not alias");
    const MapFrames f = {width, height, (uint32_t)batch, elem_size, (uint64_t)grid_pitch, (uint64_t)out_pitch,
                         (uint64_t)grid_frame_stride, (uint64_t)out_frame_stride};
    const MapJudged j = map_plan(reinterpret_cast<uintptr_t>(d_grid), f);
    const MapPlan &mp = j.plan;
    if (!mp.p.ok) return fail(HGI_EINVAL, "more tiles than a launch holds");
    // ---- HGI_EUNSUPPORTED ----
    if (levels == 0 || levels > 8)
        return fail(HGI_EUNSUPPORTED, "levels %u: one launch serves 1..=8 levels (compose decode + gather)", levels);
    if (!j.fits32)
        return fail(HGI_EUNSUPPORTED, "a side's offsets do not fit the 32-bit buffer path (pitch and height too large; compose decode + gather)");
    if (!j.tail_ok)
        return fail(HGI_EUNSUPPORTED, "width %u is not a multiple of 4 and the three tail bytes behind the last grid frame's span leave its 4-KiB page (compose decode + gather)", width);
    if (!mp.p.fast) return fail(HGI_EUNSUPPORTED, "the call does not take the buffer path (compose decode + gather)");
    uint32_t k, up;
    split_levels(levels, &k, &up);
    const hipError_t e = launch_decode_map(static_cast<const uint8_t *>(d_grid), d_table, d_out, mp, elem_size, k, up, (int)interp,
                                           static_cast<hipStream_t>(hip_stream));
    if (e != hipSuccess) return fail(HGI_EDEVICE, "HIP error %d (%s) in the mapped decode launch", (int)e, hipGetErrorString(e));
    return HGI_OK;
}

const char *hgi_map_last_error(void) { return g_err; }

const char *hgi_map_version(void) { return "hgi_map 1.0 (HIP, gfx950: mapped decode)"; }

}  // extern "C"
