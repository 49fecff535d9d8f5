// C ABI of libhgi_recon.so (include/hgi_recon.h): encode with reconstruction.  Argument rules, the three-sided plan
// (hgi_recon_plan.h) and the one launch (hgi_fused_recon_enc.hip).  Stateless: no ctx, no scratch, no environment.
// Every argument rule is decided before the first HIP call.
#include <hip/hip_runtime.h>
#include <string.h>

#include "../../include/hgi_recon.h"
#include "../companion/hgi_entry.h"
#include "hgi_recon_kernels.h"

using namespace hgi;

extern "C" {

hgi_status hgi_recon_encode_u8_dev(void *hip_stream, const void *d_img, size_t img_pitch, uint32_t width, uint32_t height,
                                   uint32_t levels, hgi_interp interp, const uint8_t lut[256], void *d_grid, size_t grid_pitch,
                                   void *d_recon, size_t recon_pitch, size_t batch, size_t img_frame_stride,
                                   size_t grid_frame_stride, size_t recon_frame_stride)
{
    typedef unsigned __int128 u128;
    // an empty call succeeds and does nothing, whatever its other arguments
    if (width == 0 || height == 0 || batch == 0) return HGI_OK;
    if (levels > 31) return fail(HGI_EINVAL, "levels %u out of range 0..=31", levels);
    if (interp != HGI_INTERP_LEFTTOP && interp != HGI_INTERP_CROSSED)
        return fail(HGI_EUNSUPPORTED, "interpolator %d not implemented (0 = LeftTop, 1 = Crossed)", (int)interp);
    if (!lut) return fail(HGI_EINVAL, "lut is NULL");
    if (levels == 0 || levels > 8)
        return fail(HGI_EUNSUPPORTED, "levels %u: one launch serves 1..=8 levels (compose encode + decode)", levels);
    if (!d_img || !d_grid || !d_recon) return fail(HGI_EINVAL, "NULL buffer");
    if (img_pitch < width) return fail(HGI_EINVAL, "image pitch %zu < width %u", img_pitch, width);
    if (grid_pitch < width) return fail(HGI_EINVAL, "grid pitch %zu < width %u", grid_pitch, width);
    if (recon_pitch < width) return fail(HGI_EINVAL, "reconstruction pitch %zu < width %u", recon_pitch, width);
    if (batch > 0x7fffffffu) return fail(HGI_EINVAL, "batch too large");
    const u128 ispan = (u128)(height - 1) * img_pitch + width, gspan = (u128)(height - 1) * grid_pitch + width,
               rspan = (u128)(height - 1) * recon_pitch + width;
    if (batch > 1 && (u128)img_frame_stride < ispan)
        return fail(HGI_EINVAL, "image frame stride %zu < (height - 1) * pitch + width", img_frame_stride);
    if (batch > 1 && (u128)grid_frame_stride < gspan)
        return fail(HGI_EINVAL, "grid frame stride %zu < (height - 1) * pitch + width", grid_frame_stride);
    if (batch > 1 && (u128)recon_frame_stride < rspan)
        return fail(HGI_EINVAL, "reconstruction frame stride %zu < (height - 1) * pitch + width", recon_frame_stride);
    // No aliasing, tested conservatively: the byte intervals the three sides span must not meet.
    const Interval ii = side_interval(reinterpret_cast<uintptr_t>(d_img), width, height, img_pitch, img_frame_stride, batch);
    const Interval gi = side_interval(reinterpret_cast<uintptr_t>(d_grid), width, height, grid_pitch, grid_frame_stride, batch);
    const Interval ri = side_interval(reinterpret_cast<uintptr_t>(d_recon), width, height, recon_pitch, recon_frame_stride, batch);
    if (ii.hi - ii.lo > (u128)SIZE_MAX || gi.hi - gi.lo > (u128)SIZE_MAX || ri.hi - ri.lo > (u128)SIZE_MAX)
        return fail(HGI_EINVAL, "frame span too large");
    if (d_recon == d_img) return fail(HGI_EINVAL, "in-place (d_recon == d_img) is refused: a tile's halo reads its neighbours' original pixels (the spans overlap)");
    if (meet(ii, gi)) return fail(HGI_EINVAL, "the grid span overlaps the image span: they must not alias");
    if (meet(ii, ri)) return fail(HGI_EINVAL, "the reconstruction span overlaps the image span: they must not alias");
    if (meet(gi, ri)) return fail(HGI_EINVAL, "the reconstruction span overlaps the grid span: they must not alias");
    const ReconFrames f = {width, height, (uint32_t)batch, (uint64_t)img_pitch, (uint64_t)grid_pitch, (uint64_t)recon_pitch,
                           (uint64_t)img_frame_stride, (uint64_t)grid_frame_stride, (uint64_t)recon_frame_stride};
    const ReconJudged j = recon_plan(reinterpret_cast<uintptr_t>(d_img), f);
    const ReconPlan &rp = j.plan;
    if (!rp.p.ok) return fail(HGI_EINVAL, "more tiles than a launch holds");
    if (!j.fits32)
        return fail(HGI_EUNSUPPORTED, "a side's offsets do not fit the 32-bit buffer path (pitch and height too large; compose encode + decode)");
    if (!j.tail_ok)
        return fail(HGI_EUNSUPPORTED, "width %u is not a multiple of 4 and the three tail bytes behind the last image frame's span leave its 4-KiB page (compose encode + decode)", width);
    if (!rp.p.fast) return fail(HGI_EUNSUPPORTED, "the call does not take the buffer path (compose encode + decode)");
    Lut256 l;
    memcpy(l.w, lut, 256);
    bool ident = true;
    for (int i = 0; i < 256; ++i) ident = ident && lut[i] == i;
    uint32_t k, up;
    split_levels(levels, &k, &up);
    const hipError_t e = launch_encode_recon(static_cast<const uint8_t *>(d_img), static_cast<uint8_t *>(d_grid),
                                             static_cast<uint8_t *>(d_recon), rp, k, up, (int)interp, l, ident,
                                             static_cast<hipStream_t>(hip_stream));
    if (e != hipSuccess) return fail(HGI_EDEVICE, "HIP error %d (%s) in the reconstruction launch", (int)e, hipGetErrorString(e));
    return HGI_OK;
}

const char *hgi_recon_last_error(void) { return g_err; }

const char *hgi_recon_version(void) { return "hgi_recon 1.0 (HIP, gfx950: encode with reconstruction)"; }

}  // extern "C"
