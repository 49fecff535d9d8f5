/*
 * hgi_recon.h -- C ABI of libhgi_recon.so: encode with reconstruction on the MI355X.
 *
 * A companion of libhgi_hip.so (hgi.h) for a capability the reference crate has no call for: the grid
 * AND the image the decoder will make of it, from ONE launch.  The reference returns the reconstruction
 * for free -- Encoder::encode overwrites its input with it (src/encoder.rs:63-64) -- and every closed
 * loop wants it: rate/quality search, `hgi test`-style reports, difference coding against the previous
 * decoded frame.  With hgi.h alone that is hgi_encode_u8_dev + hgi_decode_u8_dev: two launches, 4 B/px
 * of memory traffic.  Here it is one launch and 3 B/px.
 *
 * This header takes hgi_status and hgi_interp from hgi.h and nothing else; the library links nothing of
 * libhgi_hip.so, keeps no state (no ctx, no scratch, no device allocation) and reads no environment
 * variable.  There is NO CPU fallback and no byte-checked path: what the one launch cannot serve is
 * refused with HGI_EUNSUPPORTED and the caller composes hgi_encode_u8_dev + hgi_decode_u8_dev.
 */
#ifndef HGI_RECON_H_
#define HGI_RECON_H_

#include <stddef.h>
#include <stdint.h>

#include "hgi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- encode with reconstruction: image read, grid and reconstruction written, a pitch on each side -- */
/* Row y of frame f lies at base + f * frame_stride + y * pitch, `width` bytes, on each of the THREE      */
/* sides: pitch >= width, a pitch and a frame stride of its own per side (crops, canvas windows, padded   */
/* planes, as for the *_pitched calls of hgi.h; all three pitches == width is the packed case).           */
/*  - Grid frame f, read through its pitch, is bit for bit what hgi_encode_u8_dev writes for the packed   */
/*    copy of image f; recon frame f is bit for bit what hgi_decode_u8_dev writes for that grid.          */
/*  - ONLY the `width` bytes of each output row are written, on both outputs: the bytes between rows,     */
/*    between frames and around the spans keep their values.  The input is never modified.                */
/*  - Async on `hip_stream` (a hipStream_t; NULL = the default stream).  The calling thread's current     */
/*    device must be the stream's device.  `lut` is HOST memory, 256 bytes, copied into the launch: the   */
/*    caller may reuse it at once.  The identity table (lut[i] == i) runs a residual-only instantiation   */
/*    in the same launch and writes the image's own bytes as the reconstruction.                          */
/*  - Exactly ONE launch, for levels 1 ... 8: up to five levels the 128 x 64 tile holds the pyramid, at   */
/*    six to eight the tile kernel rebuilds the levels above a tile for itself (the cone), as the         */
/*    pitched encoder of libhgi_hip.so does.  No scratch; capturable into a graph.                        */
/*  - Reads stay inside each input frame's span [p, p + (height - 1) * pitch + width), plus at most       */
/*    three bytes behind the last frame's span when width is not a multiple of 4 (see below).  Gap bytes  */
/*    inside a span may be read; their values never influence the result.                                 */
/* HGI_EUNSUPPORTED (message in hgi_recon_last_error(), NOTHING written; compose encode + decode):        */
/*  - levels == 0 or 9 <= levels <= 31; an interp other than the two of hgi_interp;                       */
/*  - a side whose offsets do not fit the 32-bit buffer path: with P the largest of the three pitches     */
/*    (a one-row frame's pitch counts as width), P >= 2^32 or (height + 192) * P + 1024 >= 2^32;          */
/*  - width % 4 != 0 and the three bytes behind the last input frame's span not all in the 4-KiB page of  */
/*    the span's last byte: with end = d_img + (batch - 1) * img_frame_stride + (height - 1) * img_pitch  */
/*    + width (for batch == 1 the stride term is 0), the call is served iff                                */
/*    (end - 1) >> 12 == (end + 2) >> 12.  A caller evaluates this from its own addresses.                */
/* HGI_EINVAL:                                                                                            */
/*  - NULL lut; a NULL d_img, d_grid or d_recon of a non-empty call; levels > 31;                         */
/*  - a pitch < width; when batch > 1 a frame stride < (height - 1) * pitch + width of its side;          */
/*  - more tiles than a launch holds (ceil(width / 128) * ceil(height / 64) * batch >= 2^31 - 8);         */
/*  - aliasing, tested conservatively on byte spans as for the pitched calls: no two of the three         */
/*    intervals [p, p + (batch - 1) * frame_stride + span) may meet.  In-place (d_recon == d_img) is      */
/*    refused with them: a tile's halo reads its neighbours' ORIGINAL pixels.                             */
/* batch == 0, width == 0 or height == 0 succeeds and does nothing: that is decided first, so an empty    */
/* call returns HGI_OK whatever its other arguments are.  Every argument rule is decided before the       */
/* first HIP call.  A failed launch returns HGI_EDEVICE.                                                  */
HGI_API hgi_status hgi_recon_encode_u8_dev(void *hip_stream, const void *d_img, size_t img_pitch, uint32_t width,
                                           uint32_t height, uint32_t levels, hgi_interp interp, const uint8_t lut[256],
                                           void *d_grid, size_t grid_pitch, void *d_recon, size_t recon_pitch, size_t batch,
                                           size_t img_frame_stride, size_t grid_frame_stride, size_t recon_frame_stride);

/* Thread-local message of the calling thread's last failed hgi_recon_* call (like hgi_last_error). */
HGI_API const char *hgi_recon_last_error(void);

/* Library version; names the GPU architecture it was built for (gfx950). */
HGI_API const char *hgi_recon_version(void);

#ifdef __cplusplus
}
#endif

#endif /* HGI_RECON_H_ */
