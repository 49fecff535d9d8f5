/*
 * hgi_sviews.h -- C ABI of libhgi_sviews.so: scaled view lists, stored grids of different shapes decoded at
 * 1 / 2^s resolution, each with a read pitch and a write pitch of its own, in ONE launch on the MI355X.
 *
 * A companion of libhgi_hip.so (hgi.h).  Scaled decode (hgi_decode_scaled_u8_dev) writes the stride-2^s
 * lattice of the full decode from the grid bytes of that lattice alone, but one shape per call and packed
 * grids only; the view lists (hgi_views.h) decode grids of different shapes in one launch, but at full
 * resolution.  Here every grid of a call brings {pointer, row pitch, size} for the grid that is read and
 * {pointer, row pitch} for the image of ceil(width / 2^s) x ceil(height / 2^s) bytes that is written: every
 * grid of a ragged store at 1/2, 1/4 or 1/8 resolution -- a gallery of previews -- at the bytes of that
 * lattice.
 *
 * PLAN ONCE, LAUNCH MANY, as in hgi_views.h: hgi_sviews_plan is pure host code, judges every rule of the
 * list and writes a position-independent blob into caller memory and a small host struct; the caller
 * uploads the blob and hands its device address to any number of launches.  A launch is exactly one
 * kernel launch with nothing else on the stream: stateless and capturable into a graph.  The plan depends
 * on the shift, not on the depth or the interpolator.
 *
 * This header takes hgi_status and hgi_interp from hgi.h; the library links nothing of libhgi_hip.so,
 * keeps no state (no ctx, no scratch, no device allocation) and reads no environment variable.  There is
 * NO CPU fallback and no byte-checked path: what the one launch cannot serve is refused with
 * HGI_EUNSUPPORTED and the caller composes one hgi_decode_scaled_u8_dev call per view.
 *
 * THIS LIBRARY HAS NO PAGE RULE.  A launch reads nothing outside the grids' byte spans
 * [src, src + (height - 1) * src_pitch + width): every load goes through a descriptor whose range is the
 * span.  Inside a span it may read gap bytes and bytes off the stride-2^s lattice; their values never
 * influence a result.
 */
#ifndef HGI_SVIEWS_H_
#define HGI_SVIEWS_H_

#include <stddef.h>
#include <stdint.h>

#include "hgi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One grid of a call.  Row y of the grid lies at src + y * src_pitch, `width` bytes; row j of the image  */
/* at dst + j * dst_pitch, sw = ceil(width / 2^s) bytes, sh = ceil(height / 2^s) rows.                    */
typedef struct hgi_sview_pair {
    uint64_t src, dst;             /* device addresses: the stored grid, the scaled image */
    uint32_t width, height;        /* of the GRID, pixels; a zero in either skips the entry */
    uint64_t src_pitch, dst_pitch; /* bytes between rows (a one-row side's pitch is not looked at) */
} hgi_sview_pair;

#define HGI_SVIEWS_MAGIC 0x56534731u /* "1GSV" */

/* What hgi_sviews_plan tells the launch about the blob it wrote (host memory, filled by the plan only):  */
/* hgi_views_info's layout with a magic of its own and the shift in its reserved slot.                    */
typedef struct hgi_sviews_info {
    uint32_t magic;                /* HGI_SVIEWS_MAGIC */
    uint32_t count;                /* non-empty grids = records in the blob */
    uint32_t edge_tiles;           /* ragged 128 x 64 tiles of the OUTPUT images over the list */
    uint32_t interior_tiles;       /* tiles whose body lies inside their image and whose wide loads stay in the grid's span */
    uint32_t max_width;            /* the widest output image (sw) */
    uint32_t shift;                /* the s the plan was made for: 1 ... 31 (0: a plan of no entry made without one) */
    uint64_t plan_bytes;           /* bytes of the blob in use: upload these */
    uint64_t records_offset;       /* count records of 64 bytes */
    uint64_t edge_prefix_offset;   /* count uint32: ragged tiles of the grids in front of each */
    uint64_t interior_prefix_offset; /* count uint32: interior tiles of the grids in front of each */
} hgi_sviews_info;

/* Bytes a plan of n entries needs at most (h_plan of hgi_sviews_plan; the upload is info->plan_bytes).   */
HGI_API size_t hgi_sviews_plan_bytes(size_t n);

/* ---- the plan: every argument rule of a list, decided on the host, without a HIP call ---------------- */
/*  - Writes the blob to h_plan (plan_bytes >= hgi_sviews_plan_bytes(n)) and fills *info.  On a refusal   */
/*    info->magic is 0, the blob is untouched and no launch accepts the info.  n == 0: HGI_OK whatever    */
/*    the other arguments; only empty entries: HGI_OK, info->count == 0; a launch of such a plan succeeds */
/*    and does nothing.  Every rule is decided before anything is written.                                */
/*  - The blob holds addresses and sizes, no host pointer: copy it to the device (16-byte aligned) and    */
/*    keep it unchanged while launches that read it are in flight.  Device code never writes it.  A blob  */
/*    MODIFIED AFTER PLANNING IS UNDEFINED BEHAVIOUR: the launch validates `info`, not the device bytes.  */
/* With sw = ceil(width / 2^shift), sh = ceil(height / 2^shift) and span = (height - 1) * src_pitch +     */
/* width (a one-row grid's: width):                                                                       */
/* HGI_EINVAL, decided before the HGI_EUNSUPPORTED rules, in this order (the text names the list index):  */
/*  - a NULL views, h_plan or info of a non-empty call; plan_bytes too small; shift > 31;                 */
/*  - per non-empty entry, in list order: a NULL src or dst; src_pitch < width where height > 1;          */
/*    dst_pitch < sw where sh > 1;                                                                        */
/*  - more tiles than a launch holds (the 128 x 64 tiles of all OUTPUT images, padded, + 8 >= 2^31);      */
/*  - aliasing, on RECTANGLES OF BYTES exactly as in hgi_views.h.  The input rectangle of an entry is the */
/*    whole grid, width x height at src_pitch (the launch may read any byte of it); the output rectangle  */
/*    is sw x sh at dst_pitch.  Grids may overlap each other; outputs must be pairwise disjoint, and no   */
/*    output may meet a grid.  Two rectangles whose byte spans meet are judged exactly when they have the */
/*    same pitch or one of them is a single row; spans of two rectangles of more than one row that meet   */
/*    with DIFFERENT pitches are refused, conservatively.                                                 */
/* HGI_EUNSUPPORTED (NOTHING written; compose one hgi_decode_scaled_u8_dev call per view):                */
/*  - shift == 0: that is hgi_views_plan's list;                                                          */
/*  - an entry, in list order, that does not take the 32-bit buffer path on either side.  Read side: with */
/*    rp = src_pitch * 2^shift where sh > 1 and rp = span where sh == 1 (a view of one output row has no  */
/*    pitch to bound), tx = ceil(sw / 128), ty = ceil(sh / 64), the entry is served iff span < 2^32 and   */
/*    (ty * 64 + 64) * rp + (tx * 128 + 80) * 2^shift + 64 < 2^32.  Written side: with P = dst_pitch      */
/*    where sh > 1 and P = sw where sh == 1, iff P < 2^32 and (sh + 192) * P + 1024 < 2^32.               */
/*    (The read bound holds a whole tile's columns at 2^shift bytes each: no shift above 24 is served.)   */
/* Which tiles are interior (info->interior_tiles; it changes the speed of a launch, never its result):   */
/* the first sw / 128 by sh / 64 tiles of an image -- fewer rows of them when a wide load on the grid's   */
/* last lattice row would leave the span, (sh - 1) * rp + (sw / 128) * 128 * 2^shift > span: then tile    */
/* rows that reach that row, (iy - 1) * 64 + 96 >= sh - 1, are ragged, whatever the depth of a launch.    */
HGI_API hgi_status hgi_sviews_plan(const hgi_sview_pair *views, size_t n, uint32_t shift, void *h_plan, size_t plan_bytes,
                                   hgi_sviews_info *info);

/* ---- the launch -------------------------------------------------------------------------------------- */
/*  - Byte (i, j) of output view n is bit for bit byte (i * 2^s, j * 2^s) of                              */
/*    hgi_decode_u8_dev(packed copy of grid n, levels, interp), s = info->shift.  ONLY the sw bytes of    */
/*    each output row are written; the grids and the blob are never written.                              */
/*  - Async on `hip_stream` (a hipStream_t; NULL = the default stream); the calling thread's current      */
/*    device must be the stream's.  d_plan: the device copy of the blob, 16-byte aligned.  Exactly ONE    */
/*    kernel launch: with r = levels - s remaining levels, up to five the 128 x 64 tile holds the         */
/*    pyramid; at six to eight the tile rebuilds the levels above it from its grid's own lattice samples  */
/*    through the pitch.  No scratch; capturable into a graph.                                            */
/*  - A plan of no non-empty grid (info->count == 0, magic set): HGI_OK, nothing launched, decided first. */
/* HGI_EINVAL, before the HGI_EUNSUPPORTED rules, in this order: a NULL info; an `info` that is           */
/* inconsistent (magic, shift, the sizes and offsets against the count, the block count); a NULL or       */
/* misaligned d_plan; levels > 31; an unknown interpolator.  HGI_EUNSUPPORTED, in this order:             */
/* levels == 0; levels <= shift (the result is the grid's own lattice: a strided gather, for which this   */
/* library has no kernel); levels - shift >= 9.  A failed launch returns HGI_EDEVICE.                     */
HGI_API hgi_status hgi_sviews_decode_dev(void *hip_stream, const void *d_plan, const hgi_sviews_info *info, uint32_t levels,
                                         hgi_interp interp);

/* Thread-local message of the calling thread's last failed hgi_sviews_* call (like hgi_last_error). */
HGI_API const char *hgi_sviews_last_error(void);

/* Library version; names the GPU architecture it was built for (gfx950). */
HGI_API const char *hgi_sviews_version(void);

#ifdef __cplusplus
}
#endif

#endif /* HGI_SVIEWS_H_ */
