/*
 * hgi_views.h -- C ABI of libhgi_views.so: view lists, frames with a pitch of their own each, coded in
 * ONE launch on the MI355X.
 *
 * A companion of libhgi_hip.so (hgi.h).  The frame lists of hgi.h code mixed-size frames in one launch,
 * but only packed ones; the pitched calls code frames where they lie, but one shape and one pitch pair
 * per call.  Here every frame of a call brings {pointer, row pitch, size} for the side that is read and
 * for the side that is written: sprites in an atlas, the tiles of a mosaic decoded into their places on
 * one canvas, crops of different sizes out of one device image, mixed-size planes with padded rows.
 *
 * PLAN ONCE, LAUNCH MANY.  hgi_views_plan is pure host code: it judges every rule of the list and writes
 * a position-independent blob (records and prefix arrays, addressed by offsets) into caller memory, and
 * a small host struct.  The caller uploads the blob wherever it likes and hands its device address to
 * any number of launches.  A launch is exactly one kernel launch with nothing else on the stream: it is
 * stateless and capturable into a graph.  The plan depends on neither direction nor depth; `src` is
 * always the side that is READ (the image of an encode, the grid of a decode).
 *
 * This header takes hgi_status and hgi_interp from hgi.h; the library links nothing of libhgi_hip.so,
 * keeps no state (no ctx, no scratch, no device allocation) and reads no environment variable.  There is
 * NO CPU fallback and no byte-checked path: what the one launch cannot serve is refused with
 * HGI_EUNSUPPORTED and the caller composes one hgi_*_u8_pitched_dev call per view.
 */
#ifndef HGI_VIEWS_H_
#define HGI_VIEWS_H_

#include <stddef.h>
#include <stdint.h>

#include "hgi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One frame of a call: where it is read, where it is written.  Row y lies at base + y * pitch, `width`  */
/* bytes, on each side.                                                                                   */
typedef struct hgi_view_pair {
    uint64_t src, dst;             /* device addresses */
    uint32_t width, height;        /* pixels; a zero in either skips the entry */
    uint64_t src_pitch, dst_pitch; /* bytes between rows, >= width (a one-row frame's pitch counts as width) */
} hgi_view_pair;

#define HGI_VIEWS_MAGIC 0x56494731u /* "1GIV" */

/* What hgi_views_plan tells the launches about the blob it wrote (host memory, filled by the plan only). */
typedef struct hgi_views_info {
    uint32_t magic;                /* HGI_VIEWS_MAGIC */
    uint32_t count;                /* non-empty frames = records in the blob */
    uint32_t edge_tiles;           /* ragged 128 x 64 tiles over the list */
    uint32_t interior_tiles;       /* tiles whose body lies inside their frame */
    uint32_t max_width;            /* the widest frame */
    uint32_t reserved;             /* 0 */
    uint64_t plan_bytes;           /* bytes of the blob in use: upload these */
    uint64_t records_offset;       /* count records of 64 bytes */
    uint64_t edge_prefix_offset;   /* count uint32: ragged tiles of the frames in front of each */
    uint64_t interior_prefix_offset; /* count uint32: interior tiles of the frames in front of each */
} hgi_views_info;

/* Bytes a plan of n entries needs at most (h_plan of hgi_views_plan; the upload is info->plan_bytes).   */
HGI_API size_t hgi_views_plan_bytes(size_t n);

/* ---- the plan: every argument rule of a list, decided on the host, without a HIP call ---------------- */
/*  - Writes the blob to h_plan (plan_bytes >= hgi_views_plan_bytes(n)) and fills *info.  On a refusal    */
/*    info->magic is 0 and no launch accepts it.  n == 0 or only empty entries: HGI_OK, info->count == 0, */
/*    and a launch of that plan succeeds and does nothing.                                                */
/*  - The blob holds addresses and sizes, no host pointer: copy it to the device (16-byte aligned) and    */
/*    keep it unchanged while launches that read it are in flight.  Device code never writes it.  A blob  */
/*    MODIFIED AFTER PLANNING IS UNDEFINED BEHAVIOUR, as a wrong pointer is: the launch validates `info`, */
/*    not the device bytes.                                                                               */
/* HGI_EINVAL, decided before the HGI_EUNSUPPORTED rules (the text names the offending list index):       */
/*  - a NULL views, h_plan or info of a non-empty call; plan_bytes too small;                             */
/*  - a NULL src or dst of a non-empty entry; a pitch < width;                                            */
/*  - more tiles than a launch holds (the 128 x 64 tiles of all entries, padded, + 8 >= 2^31);            */
/*  - aliasing.  Inputs may overlap each other (two crops of one image).  Outputs must be pairwise        */
/*    disjoint AS RECTANGLES OF BYTES, and no output may meet an input -- in place is refused with that:  */
/*    a tile's halo reads its neighbours' originals.  Views whose byte spans                              */
/*    [p, p + (height - 1) * pitch + width) do not meet are fine.  Two views whose spans meet are judged  */
/*    exactly when both have the same pitch P: with the lower address as origin the other view starts at  */
/*    column (b - a) mod P, row (b - a) / P; the pair is fine iff that column plus its width is <= P and  */
/*    the two rectangles are disjoint (windows side by side in one parent's rows).  A one-row view is an  */
/*    interval of bytes and is judged exactly against any other view.  Spans of two views of more than    */
/*    one row that meet with DIFFERENT pitches are refused, conservatively.                               */
/* HGI_EUNSUPPORTED (NOTHING written; compose one hgi_*_u8_pitched_dev call per view):                    */
/*  - an entry whose offsets do not fit the 32-bit buffer path: with P the larger of its two pitches,     */
/*    P >= 2^32 or (height + 192) * P + 1024 >= 2^32;                                                     */
/*  - an entry with width % 4 != 0 whose three bytes behind ITS OWN source span leave the 4-KiB page of   */
/*    the span's last byte: with end = src + (height - 1) * src_pitch + width the entry is served iff     */
/*    (end - 1) >> 12 == (end + 2) >> 12.                                                                 */
/* What a launch may READ beyond the width bytes of the source rows: gap bytes inside a source span, and  */
/* at most three bytes behind a view's last row when its width is not a multiple of 4.  Their values      */
/* never influence a result, even if another view of the same call is writing them.                      */
HGI_API hgi_status hgi_views_plan(const hgi_view_pair *views, size_t n, void *h_plan, size_t plan_bytes, hgi_views_info *info);

/* ---- the launches ------------------------------------------------------------------------------------ */
/*  - Output view i, read through its pitch, is bit for bit what hgi_encode_u8_dev / hgi_decode_u8_dev    */
/*    writes for the packed copy of input view i alone.  ONLY the `width` bytes of each output row are    */
/*    written; inputs are never modified.                                                                 */
/*  - Async on `hip_stream` (a hipStream_t; NULL = the default stream); the calling thread's current      */
/*    device must be the stream's.  `lut` is HOST memory, 256 bytes, copied into the launch.  d_plan: the */
/*    device copy of the blob, 16-byte aligned.  Exactly ONE kernel launch for levels 1 ... 8 (up to five */
/*    levels the 128 x 64 tile holds the pyramid; at six to eight the tile rebuilds the levels above it   */
/*    from its frame's own samples through the pitch).  No scratch; capturable into a graph.              */
/*  - A plan of no non-empty frame (info->count == 0, magic set): HGI_OK, nothing launched, decided first.*/
/* HGI_EINVAL, before the HGI_EUNSUPPORTED rule: a NULL info; an `info` that is inconsistent (magic, the  */
/* sizes and offsets against the count, the block count); a NULL or misaligned d_plan; a NULL lut;        */
/* levels > 31; an unknown interpolator.  HGI_EUNSUPPORTED: levels == 0 or 9 <= levels <= 31.  A failed   */
/* launch returns HGI_EDEVICE.                                                                            */
HGI_API hgi_status hgi_views_encode_dev(void *hip_stream, const void *d_plan, const hgi_views_info *info, uint32_t levels,
                                        hgi_interp interp, const uint8_t *lut);
HGI_API hgi_status hgi_views_decode_dev(void *hip_stream, const void *d_plan, const hgi_views_info *info, uint32_t levels,
                                        hgi_interp interp);

/* Thread-local message of the calling thread's last failed hgi_views_* call (like hgi_last_error). */
HGI_API const char *hgi_views_last_error(void);

/* Library version; names the GPU architecture it was built for (gfx950). */
HGI_API const char *hgi_views_version(void);

#ifdef __cplusplus
}
#endif

#endif /* HGI_VIEWS_H_ */
