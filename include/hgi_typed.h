/*
 * hgi_typed.h -- C ABI of libhgi_typed.so: typed encode on the MI355X.
 *
 * A companion of libhgi_hip.so (hgi.h) and the way in that goes with hgi_map.h's way out: frames of
 * float16, bfloat16 or float32 elements, normalised or not, encoded into grids by ONE launch.  With
 * hgi.h alone that is an elementwise conversion to uint8 plus hgi_encode_u8_pitched_dev: two launches,
 * (E + 1 + 1 + 1) B/px of memory traffic.  Here it is one launch and (E + 1) B/px, and the uint8 image
 * never exists in memory.
 *
 * The conversion, for an element x (float16 / bfloat16 widened exactly to float32, or float32) and the
 * two float32 launch constants `scale` and `bias`:
 *     t = fl32(fl32(x * scale) + bias)     two separately rounded float32 operations, never an fma
 *     v = 0                                if t is NaN
 *     v = clamp(rint(t), 0, 255)           otherwise; rint rounds half to even; +-inf clamp
 * Denormals are not flushed, in x or in t.  The pixel the codec encodes is v.
 *
 * This header takes hgi_status and hgi_interp from hgi.h and nothing else; the library links nothing of
 * libhgi_hip.so, keeps no state (no ctx, no scratch, no device allocation) and reads no environment
 * variable.  There is NO CPU fallback and no byte-checked path: what the one launch cannot serve is
 * refused with HGI_EUNSUPPORTED and the caller composes a conversion + hgi_encode_u8_pitched_dev.
 */
#ifndef HGI_TYPED_H_
#define HGI_TYPED_H_

#include <stddef.h>
#include <stdint.h>

#include "hgi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- typed encode: frames of elem_size-byte elements read through a pitch, grids written -------------- */
/* Image row y of frame f lies at d_img + f * img_frame_stride + y * img_pitch, width * elem_size bytes;   */
/* grid row y of frame f lies at d_grid + f * grid_frame_stride + y * grid_pitch, `width` bytes (the       */
/* convention of hgi_encode_u8_pitched_dev).  Pitches and strides are in BYTES on both sides.              */
/*  - elem_kind 0: IEEE elements, float16 at elem_size 2 and float32 at elem_size 4; elem_kind 1:          */
/*    bfloat16 (elem_size 2 only).                                                                         */
/*  - Grid frame f, read through its pitch, is bit for bit what hgi_encode_u8_dev makes of the packed      */
/*    uint8 image that the conversion above makes of frame f.                                              */
/*  - ONLY the `width` bytes of each grid row are written: the bytes between rows, between frames and      */
/*    around the span keep their values.  The input is never modified.                                     */
/*  - `lut` is HOST memory, 256 bytes, copied into the launch.  The identity table runs a residual-only    */
/*    instantiation, as in hgi_recon.h.                                                                    */
/*  - Async on `hip_stream` (a hipStream_t; NULL = the default stream).  The calling thread's current      */
/*    device must be the stream's device.                                                                  */
/*  - Exactly ONE launch, for levels 1 ... 8: up to five levels the 128 x 64 tile holds the pyramid, at    */
/*    six to eight the tile kernel rebuilds the levels above a tile for itself (the cone), as the pitched  */
/*    encoder of libhgi_hip.so does.  No scratch; capturable into a graph.                                 */
/*  - Reads of the image stay inside each frame's span [p, p + (height - 1) * pitch + width * elem_size),  */
/*    at elem_size 4 without exception: the dwords of 4-byte-aligned elements never straddle its end.  At  */
/*    elem_size 2 and an ODD width the dword that holds the last element of the last row does, and the two */
/*    bytes behind the last frame's span are read with it (the page rule below).  Gap bytes inside a span  */
/*    may be read and hold anything, NaN and infinity included; their values never influence the result.   */
/* HGI_EINVAL:                                                                                             */
/*  - a NULL lut; a NULL d_img or d_grid of a non-empty call; levels > 31;                                 */
/*  - elem_size other than 2 or 4; elem_kind > 1, or bfloat16 at elem_size 4;                              */
/*  - d_img, img_pitch or (batch > 1) img_frame_stride not a multiple of elem_size;                        */
/*  - img_pitch < width * elem_size, grid_pitch < width; when batch > 1 a frame stride below its side's    */
/*    span, (height - 1) * pitch + width [* elem_size];                                                    */
/*  - batch >= 2^31; more tiles than a launch holds (ceil(width / 128) * ceil(height / 64) * batch >=      */
/*    2^31 - 8);                                                                                           */
/*  - aliasing, tested conservatively on byte intervals: the image's [p, p + (batch - 1) * frame_stride +  */
/*    span) and the grid's likewise must be disjoint;                                                      */
/*  - a scale or bias that is not finite.                                                                  */
/* HGI_EUNSUPPORTED (message in hgi_typed_last_error(), NOTHING written; compose conversion + encode):     */
/*  - levels == 0 or 9 <= levels <= 31;                                                                    */
/*  - a side whose offsets do not fit the 32-bit buffer path: with P the larger of img_pitch and           */
/*    grid_pitch, both in bytes (a one-row frame's pitch counts as its row: width * elem_size, width),     */
/*    P >= 2^32 or (height + 192) * P + 1024 >= 2^32;                                                      */
/*  - an interp other than the two of hgi_interp;                                                          */
/*  - the page rule: elem_size 2, an odd width, and the two bytes behind the last image frame's span not   */
/*    in the 4-KiB page of the span's last byte: with end = d_img + (batch - 1) * img_frame_stride +       */
/*    (height - 1) * img_pitch + 2 * width (for batch == 1 the stride term is 0; for height == 1 the pitch */
/*    term), the call is served iff (end - 1) >> 12 == (end + 1) >> 12, i.e. iff end is not a multiple of  */
/*    4096.  A caller evaluates this from its own addresses.                                               */
/* batch == 0, width == 0 or height == 0 succeeds and does nothing: that is decided first, so an empty     */
/* call returns HGI_OK whatever its other arguments are.  Every argument rule is decided before the first  */
/* HIP call, the HGI_EINVAL rules before the HGI_EUNSUPPORTED ones.  A failed launch returns HGI_EDEVICE.  */
HGI_API hgi_status hgi_typed_encode_dev(void *hip_stream, const void *d_img, size_t img_pitch, uint32_t elem_size,
                                        uint32_t elem_kind, float scale, float bias, uint32_t width, uint32_t height,
                                        uint32_t levels, hgi_interp interp, const uint8_t lut[256], void *d_grid,
                                        size_t grid_pitch, size_t batch, size_t img_frame_stride, size_t grid_frame_stride);

/* Thread-local message of the calling thread's last failed hgi_typed_* call (like hgi_last_error). */
HGI_API const char *hgi_typed_last_error(void);

/* Library version; names the GPU architecture it was built for (gfx950). */
HGI_API const char *hgi_typed_version(void);

#ifdef __cplusplus
}
#endif

#endif /* HGI_TYPED_H_ */
