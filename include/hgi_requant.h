/*
 * hgi_requant.h -- C ABI of libhgi_requant.so: grids re-coded with another quantizer on the MI355X.
 *
 * A companion of libhgi_hip.so (hgi.h).  A grid stores dequantized residuals, so the quantizer is a
 * property of the encode alone and changing the rate of stored grids -- Lossless to Medium for an archive
 * tier, Medium to High for a thumbnail store -- is hgi_decode_u8_dev followed by hgi_encode_u8_dev with
 * the new table: two launches, 4 B/px of memory traffic and a whole uint8 image nobody wants.  Here it is
 * one launch and 2 B/px: each tile decodes in LDS and registers and encodes from there.
 *
 * This header takes hgi_status and hgi_interp from hgi.h and nothing else; the library links nothing of
 * libhgi_hip.so, keeps no state (no ctx, no scratch, no device allocation) and reads no environment
 * variable.  There is NO CPU fallback and no byte-checked path: what the one launch cannot serve is
 * refused with HGI_EUNSUPPORTED and the caller composes hgi_decode_u8_dev + hgi_encode_u8_dev.
 */
#ifndef HGI_REQUANT_H_
#define HGI_REQUANT_H_

#include <stddef.h>
#include <stdint.h>

#include "hgi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- requantize: source grid read, new grid written, a pitch on each side ---------------------------- */
/* Row y of frame f lies at base + f * frame_stride + y * pitch, `width` bytes, on each of the TWO sides: */
/* pitch >= width, a pitch and a frame stride of its own per side (as for the *_pitched calls of hgi.h;   */
/* both pitches == width is the packed case).                                                             */
/*  - Destination frame f, read through its pitch, is bit for bit                                         */
/*        hgi_encode_u8_dev(hgi_decode_u8_dev(src_f, levels, interp), levels, interp, lut)                */
/*    on the packed copy of source frame f.                                                               */
/*  - ONE `levels` and ONE `interp` serve both directions: the source is decoded with the depth and the   */
/*    predictor it is then encoded with.  A change of depth or of predictor stays a composition by the    */
/*    caller (hgi_decode_u8_dev with the old ones, hgi_encode_u8_dev with the new).                       */
/*  - ONLY the `width` bytes of each destination row are written: the bytes between rows, between frames  */
/*    and around the spans keep their values.  The source is never modified.                              */
/*  - Async on `hip_stream` (a hipStream_t; NULL = the default stream).  The calling thread's current     */
/*    device must be the stream's device.  `lut` is HOST memory, 256 bytes, copied into the launch: the   */
/*    caller may reuse it at once.                                                                        */
/*  - Exactly ONE launch, for levels 1 ... 8: up to five levels the 128 x 64 tile holds the pyramid, at   */
/*    six to eight the tile kernel rebuilds the levels above a tile for itself (the cone), once in each   */
/*    direction.  No scratch; capturable into a graph.                                                    */
/*  - Reads stay inside each source frame's span [p, p + (height - 1) * pitch + width), plus at most      */
/*    three bytes behind the last frame's span when width is not a multiple of 4 (see below).  Gap bytes  */
/*    inside a span may be read; their values never influence the result.                                 */
/* HGI_EINVAL, decided before the HGI_EUNSUPPORTED rules:                                                 */
/*  - NULL lut; a NULL d_src or d_dst of a non-empty call; levels > 31;                                   */
/*  - a pitch < width; when batch > 1 a frame stride < (height - 1) * pitch + width of its side;          */
/*  - batch >= 2^31; more tiles than a launch holds (ceil(width / 128) * ceil(height / 64) * batch >=     */
/*    2^31 - 8);                                                                                          */
/*  - a side whose interval (below) is longer than SIZE_MAX bytes ("frame span too large");               */
/*  - aliasing, tested conservatively on byte spans as for the pitched calls: the two intervals           */
/*    [p, p + (batch - 1) * frame_stride + span) may not meet.  IN PLACE (d_dst == d_src) IS REFUSED with */
/*    them: a tile's halo reads its neighbours' SOURCE residuals, which a neighbour may have overwritten. */
/* HGI_EUNSUPPORTED (message in hgi_requant_last_error(), NOTHING written; compose decode + encode):      */
/*  - levels == 0 or 9 <= levels <= 31; an interp other than the two of hgi_interp;                       */
/*  - a side whose offsets do not fit the 32-bit buffer path: with P the larger of the two pitches        */
/*    (a one-row frame's pitch counts as width), P >= 2^32 or (height + 192) * P + 1024 >= 2^32;          */
/*  - width % 4 != 0 and the three bytes behind the last source frame's span not all in the 4-KiB page of */
/*    the span's last byte: with end = d_src + (batch - 1) * src_frame_stride + (height - 1) * src_pitch  */
/*    + width (for batch == 1 the stride term is 0), the call is served iff                               */
/*    (end - 1) >> 12 == (end + 2) >> 12.  A caller evaluates this from its own addresses.                */
/*  - the identity table (lut[i] == i for all i).  Under it the encoder keeps every residual, so encoding */
/*    a decoded grid gives the grid back: the result IS the source.  Copy the source instead; no kernel   */
/*    is built for this table.                                                                            */
/* batch == 0, width == 0 or height == 0 succeeds and does nothing: that is decided first, so an empty    */
/* call returns HGI_OK whatever its other arguments are.  Every argument rule is decided before the       */
/* first HIP call.  A failed launch returns HGI_EDEVICE.                                                  */
HGI_API hgi_status hgi_requant_dev(void *hip_stream, const void *d_src, size_t src_pitch, uint32_t width, uint32_t height,
                                   uint32_t levels, hgi_interp interp, const uint8_t lut[256], void *d_dst, size_t dst_pitch,
                                   size_t batch, size_t src_frame_stride, size_t dst_frame_stride);

/* Thread-local message of the calling thread's last failed hgi_requant_* call (like hgi_last_error). */
HGI_API const char *hgi_requant_last_error(void);

/* Library version; names the GPU architecture it was built for (gfx950). */
HGI_API const char *hgi_requant_version(void);

#ifdef __cplusplus
}
#endif

#endif /* HGI_REQUANT_H_ */
