/*
 * hgi_map.h -- C ABI of libhgi_map.so: mapped decode on the MI355X.
 *
 * A companion of libhgi_hip.so (hgi.h) for a capability the reference crate has no call for: grids
 * decoded straight into frames of 2- or 4-byte elements (float16, bfloat16, float32, ...), normalised
 * or not, from ONE launch.  A pixel has 256 values, so any conversion of a decoded byte is a table of
 * 256 output elements: out[p] = table[decoded[p]].  With hgi.h alone that is hgi_decode_u8_dev plus an
 * elementwise conversion: two launches, (2 + 1 + E) B/px of memory traffic.  Here it is one launch and
 * (1 + E) B/px.  The library moves bits and does no float arithmetic: x / 255, mean / std
 * normalisation, gamma and NaN patterns alike are whatever the caller put into the table.
 *
 * This header takes hgi_status and hgi_interp from hgi.h and nothing else; the library links nothing of
 * libhgi_hip.so, keeps no state (no ctx, no scratch, no device allocation) and reads no environment
 * variable.  There is NO CPU fallback and no byte-checked path: what the one launch cannot serve is
 * refused with HGI_EUNSUPPORTED and the caller composes hgi_decode_u8_pitched_dev + a gather.
 */
#ifndef HGI_MAP_H_
#define HGI_MAP_H_

#include <stddef.h>
#include <stdint.h>

#include "hgi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- mapped decode: grids read through a pitch, frames of elem_size-byte elements written ----------- */
/* Grid row y of frame f lies at d_grid + f * grid_frame_stride + y * grid_pitch, `width` bytes (the      */
/* convention of hgi_decode_u8_pitched_dev); output row y of frame f lies at d_out + f * out_frame_stride */
/* + y * out_pitch, width * elem_size bytes.  Pitches and strides are in BYTES on both sides.             */
/*  - Element x of output row y holds the elem_size bytes of d_table[v], v being the byte                 */
/*    hgi_decode_u8_dev writes at (x, y) for the packed copy of grid f.                                   */
/*  - ONLY the width * elem_size bytes of each output row are written: the bytes between rows, between    */
/*    frames and around the span keep their values.  The grid and the table are never modified.          */
/*  - `d_table` is DEVICE memory, 256 elements of elem_size bytes (2 or 4).  The launch reads it in       */
/*    stream order: a table overwritten on the same stream between two calls is seen by each call as it   */
/*    was queued.  It must stay valid until the launch has run.                                           */
/*  - Async on `hip_stream` (a hipStream_t; NULL = the default stream).  The calling thread's current     */
/*    device must be the stream's device.                                                                 */
/*  - Exactly ONE launch, for levels 1 ... 8: up to five levels the 128 x 64 tile holds the pyramid, at   */
/*    six to eight the tile kernel rebuilds the levels above a tile for itself (the cone), as the         */
/*    pitched decoder of libhgi_hip.so does.  No scratch; capturable into a graph.                        */
/*  - Reads of the grid stay inside each frame's span [p, p + (height - 1) * pitch + width), plus at most */
/*    three bytes behind the last frame's span when width is not a multiple of 4 (see below).  Gap bytes  */
/*    inside a span may be read; their values never influence the result.                                 */
/* HGI_EUNSUPPORTED (message in hgi_map_last_error(), NOTHING written; compose decode + gather):          */
/*  - levels == 0 or 9 <= levels <= 31;                                                                   */
/*  - a side whose offsets do not fit the 32-bit buffer path: with P the larger of grid_pitch and         */
/*    out_pitch, both in bytes (a one-row frame's pitch counts as its row: width, width * elem_size),     */
/*    P >= 2^32 or (height + 192) * P + 1024 >= 2^32;                                                     */
/*  - width % 4 != 0 and the three bytes behind the last grid frame's span not all in the 4-KiB page of   */
/*    the span's last byte: with end = d_grid + (batch - 1) * grid_frame_stride + (height - 1) *          */
/*    grid_pitch + width (for batch == 1 the stride term is 0; for height == 1 the pitch term), the call  */
/*    is served iff (end - 1) >> 12 == (end + 2) >> 12.  A caller evaluates this from its own addresses.  */
/* HGI_EINVAL:                                                                                            */
/*  - a NULL d_grid, d_table or d_out of a non-empty call; levels > 31; an interp other than the two of   */
/*    hgi_interp; elem_size other than 2 or 4;                                                            */
/*  - d_out, out_pitch or (batch > 1) out_frame_stride not a multiple of elem_size;                       */
/*  - grid_pitch < width, out_pitch < width * elem_size; when batch > 1 a frame stride below its side's   */
/*    span, (height - 1) * pitch + width [* elem_size];                                                   */
/*  - more tiles than a launch holds (ceil(width / 128) * ceil(height / 64) * batch >= 2^31 - 8);         */
/*  - aliasing, tested conservatively on byte intervals: the grid's [p, p + (batch - 1) * frame_stride +  */
/*    span), the output's likewise and the table's 256 * elem_size bytes must be pairwise disjoint.       */
/* batch == 0, width == 0 or height == 0 succeeds and does nothing: that is decided first, so an empty    */
/* call returns HGI_OK whatever its other arguments are.  Every argument rule is decided before the       */
/* first HIP call, the HGI_EINVAL rules before the HGI_EUNSUPPORTED ones.  A failed launch returns        */
/* HGI_EDEVICE.                                                                                           */
HGI_API hgi_status hgi_map_decode_dev(void *hip_stream, const void *d_grid, size_t grid_pitch, uint32_t width, uint32_t height,
                                      uint32_t levels, hgi_interp interp, const void *d_table, uint32_t elem_size, void *d_out,
                                      size_t out_pitch, size_t batch, size_t grid_frame_stride, size_t out_frame_stride);

/* Thread-local message of the calling thread's last failed hgi_map_* call (like hgi_last_error). */
HGI_API const char *hgi_map_last_error(void);

/* Library version; names the GPU architecture it was built for (gfx950). */
HGI_API const char *hgi_map_version(void);

#ifdef __cplusplus
}
#endif

#endif /* HGI_MAP_H_ */
