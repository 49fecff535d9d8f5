/*
 * hgi_mviews.h -- C ABI of libhgi_mviews.so: mapped view lists, grids of different shapes decoded straight
 * into frames of float16 / bfloat16 / float32 elements, each with a pitch of its own, in ONE launch on the
 * MI355X.
 *
 * A companion of libhgi_hip.so (hgi.h).  Mapped decode (hgi_map.h) writes out[p] = table[decoded[p]] at
 * 1 + E bytes of traffic per pixel, but one shape and one pitch pair per call; the view lists (hgi_views.h)
 * code frames of different shapes in one launch, but write bytes.  Here every frame of a call brings
 * {pointer, row pitch, size} for the grid that is read and for the frame of E-byte elements that is
 * written: a ragged batch of stored grids into a padded float tensor [N, Hmax, Wmax], or into an aligned
 * arena of float frames, normalised by the table.
 *
 * PLAN ONCE, LAUNCH MANY, as in hgi_views.h: hgi_mviews_plan is pure host code, judges every rule of the
 * list and writes a position-independent blob into caller memory and a small host struct; the caller
 * uploads the blob and hands its device address to any number of launches.  A launch is exactly one
 * kernel launch with nothing else on the stream: stateless and capturable into a graph.  The plan depends
 * on the element size, not on the depth, the interpolator or the table.
 *
 * This header takes hgi_status and hgi_interp from hgi.h; the library links nothing of libhgi_hip.so,
 * keeps no state (no ctx, no scratch, no device allocation) and reads no environment variable.  There is
 * NO CPU fallback and no byte-checked path: what the one launch cannot serve is refused with
 * HGI_EUNSUPPORTED and the caller composes one hgi_map_decode_dev call per view.
 */
#ifndef HGI_MVIEWS_H_
#define HGI_MVIEWS_H_

#include <stddef.h>
#include <stdint.h>

#include "hgi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One frame of a call.  Row y of the grid lies at src + y * src_pitch, `width` bytes; row y of the frame */
/* at dst + y * dst_pitch, `width` elements of elem_size bytes.                                           */
typedef struct hgi_mview_pair {
    uint64_t src, dst;             /* device addresses: the grid (bytes), the frame (elements) */
    uint32_t width, height;        /* pixels; a zero in either skips the entry */
    uint64_t src_pitch, dst_pitch; /* BYTES between rows on both sides (a one-row frame's pitch counts as its row) */
} hgi_mview_pair;

#define HGI_MVIEWS_MAGIC 0x564D4731u /* "1GMV" */

/* What hgi_mviews_plan tells the launch about the blob it wrote (host memory, filled by the plan only):  */
/* hgi_views_info's layout with a magic of its own, the element size, and the bounding byte interval of   */
/* all output spans.                                                                                      */
typedef struct hgi_mviews_info {
    uint32_t magic;                /* HGI_MVIEWS_MAGIC */
    uint32_t count;                /* non-empty frames = records in the blob */
    uint32_t edge_tiles;           /* ragged 128 x 64 tiles over the list */
    uint32_t interior_tiles;       /* tiles whose body lies inside their frame */
    uint32_t max_width;            /* the widest frame, pixels */
    uint32_t elem_size;            /* bytes per output element the plan was made for: 2 or 4 (0: a plan of no entry) */
    uint64_t plan_bytes;           /* bytes of the blob in use: upload these */
    uint64_t records_offset;       /* count records of 64 bytes */
    uint64_t edge_prefix_offset;   /* count uint32: ragged tiles of the frames in front of each */
    uint64_t interior_prefix_offset; /* count uint32: interior tiles of the frames in front of each */
    uint64_t dst_lo, dst_hi;       /* [dst_lo, dst_hi): the smallest byte interval that holds every output span */
} hgi_mviews_info;

/* Bytes a plan of n entries needs at most (h_plan of hgi_mviews_plan; the upload is info->plan_bytes).   */
HGI_API size_t hgi_mviews_plan_bytes(size_t n);

/* ---- the plan: every argument rule of a list, decided on the host, without a HIP call ---------------- */
/*  - Writes the blob to h_plan (plan_bytes >= hgi_mviews_plan_bytes(n)) and fills *info.  On a refusal   */
/*    info->magic is 0, the blob is untouched and no launch accepts the info.  n == 0: HGI_OK whatever    */
/*    the other arguments; only empty entries: HGI_OK, info->count == 0; a launch of such a plan succeeds */
/*    and does nothing.                                                                                   */
/*  - The blob holds addresses and sizes, no host pointer: copy it to the device (16-byte aligned) and    */
/*    keep it unchanged while launches that read it are in flight.  Device code never writes it.  A blob  */
/*    MODIFIED AFTER PLANNING IS UNDEFINED BEHAVIOUR: the launch validates `info`, not the device bytes.  */
/* HGI_EINVAL, decided before the HGI_EUNSUPPORTED rules, in this order (the text names the list index):  */
/*  - a NULL views, h_plan or info of a non-empty call; plan_bytes too small; elem_size not 2 or 4;       */
/*  - per non-empty entry, in list order: a NULL src or dst; src_pitch < width; a dst that is no multiple */
/*    of elem_size; and, for a frame of more than one row, a dst_pitch that is no multiple of elem_size   */
/*    or < width * elem_size;                                                                             */
/*  - more tiles than a launch holds (the 128 x 64 tiles of all entries, padded, + 8 >= 2^31);            */
/*  - aliasing, on RECTANGLES OF BYTES exactly as in hgi_views.h, an output rectangle being               */
/*    width * elem_size bytes wide: grids may overlap each other; outputs must be pairwise disjoint, and  */
/*    no output may meet a grid.  Two rectangles whose byte spans meet are judged exactly when they have  */
/*    the same pitch or one of them is a single row; spans of two views of more than one row that meet    */
/*    with DIFFERENT pitches are refused, conservatively.                                                 */
/* HGI_EUNSUPPORTED (NOTHING written; compose one hgi_map_decode_dev call per view):                      */
/*  - an entry whose offsets do not fit the 32-bit buffer path: with P the larger of its two BYTE         */
/*    pitches, P >= 2^32 or (height + 192) * P + 1024 >= 2^32;                                            */
/*  - an entry with width % 4 != 0 whose three bytes behind ITS OWN grid span leave the 4-KiB page of the */
/*    span's last byte: with end = src + (height - 1) * src_pitch + width the entry is served iff         */
/*    (end - 1) >> 12 == (end + 2) >> 12.                                                                 */
/* What a launch may READ beyond the width bytes of the grid rows: gap bytes inside a grid span, and at   */
/* most three bytes behind a view's last row when its width is not a multiple of 4.  Their values never   */
/* influence a result.                                                                                    */
HGI_API hgi_status hgi_mviews_plan(const hgi_mview_pair *views, size_t n, uint32_t elem_size, void *h_plan, size_t plan_bytes,
                                   hgi_mviews_info *info);

/* ---- the launch -------------------------------------------------------------------------------------- */
/*  - Output view i, read through its pitch as elements of info->elem_size bytes, is bit for bit          */
/*    table[hgi_decode_u8_dev(packed copy of grid view i)].  ONLY the width * elem_size bytes of each     */
/*    output row are written; the grids, the table and the blob are never written.                        */
/*  - d_table: DEVICE memory, 256 elements of info->elem_size bytes, at any alignment; any bit patterns.  */
/*  - Async on `hip_stream` (a hipStream_t; NULL = the default stream); the calling thread's current      */
/*    device must be the stream's.  d_plan: the device copy of the blob, 16-byte aligned.  Exactly ONE    */
/*    kernel launch for levels 1 ... 8 (up to five levels the 128 x 64 tile holds the pyramid; at six to  */
/*    eight the tile rebuilds the levels above it from its grid's own samples through the pitch).  No     */
/*    scratch; capturable into a graph.                                                                   */
/*  - A plan of no non-empty frame (info->count == 0, magic set): HGI_OK, nothing launched, decided first.*/
/* HGI_EINVAL, before the HGI_EUNSUPPORTED rule: a NULL info; an `info` that is inconsistent (magic,      */
/* elem_size, the sizes and offsets against the count, the block count, the output interval); a NULL or   */
/* misaligned d_plan; a NULL d_table; a d_table whose [d_table, d_table + 256 * elem_size) meets          */
/* [dst_lo, dst_hi) -- conservative: a table in a gap between two outputs is refused too, and the grids   */
/* are the caller's to keep apart from it, since the host cannot see the blob; levels > 31; an unknown    */
/* interpolator.  HGI_EUNSUPPORTED: levels == 0 or 9 <= levels <= 31.  A failed launch returns            */
/* HGI_EDEVICE.                                                                                           */
HGI_API hgi_status hgi_mviews_decode_dev(void *hip_stream, const void *d_plan, const hgi_mviews_info *info, uint32_t levels,
                                         hgi_interp interp, const void *d_table);

/* Thread-local message of the calling thread's last failed hgi_mviews_* call (like hgi_last_error). */
HGI_API const char *hgi_mviews_last_error(void);

/* Library version; names the GPU architecture it was built for (gfx950). */
HGI_API const char *hgi_mviews_version(void);

#ifdef __cplusplus
}
#endif

#endif /* HGI_MVIEWS_H_ */
