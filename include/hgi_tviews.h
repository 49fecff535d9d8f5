/*
 * hgi_tviews.h -- C ABI of libhgi_tviews.so: typed view lists, frames of float16 / bfloat16 / float32
 * elements of different shapes, each with a pitch of its own, encoded straight into grids in ONE launch on
 * the MI355X.
 *
 * A companion of libhgi_hip.so (hgi.h) and the way in that goes with hgi_mviews.h's way out.  Typed encode
 * (hgi_typed.h) converts v = clamp(rint(x * scale + bias), 0, 255) and encodes at E + 1 bytes of traffic
 * per pixel, but one shape and one pitch pair per call; the view lists (hgi_views.h) code frames of
 * different shapes in one launch, but read bytes.  Here every frame of a call brings {pointer, row pitch,
 * size} for the frame of E-byte elements that is read and for the grid that is written: a padded float
 * tensor [N, Hmax, Wmax] of ragged frames, an arena of float frames or float crops of one canvas, stored
 * as grids.
 *
 * PLAN ONCE, LAUNCH MANY, as in hgi_views.h: hgi_tviews_plan is pure host code, judges every rule of the
 * list and writes a position-independent blob into caller memory and a small host struct; the caller
 * uploads the blob and hands its device address to any number of launches.  A launch is exactly one
 * kernel launch with nothing else on the stream: stateless and capturable into a graph.  The plan depends
 * on the element size, not on the element kind, the conversion's constants, the depth, the interpolator
 * or the quantizer table: those belong to the launch.
 *
 * This header takes hgi_status and hgi_interp from hgi.h; the library links nothing of libhgi_hip.so,
 * keeps no state (no ctx, no scratch, no device allocation) and reads no environment variable.  There is
 * NO CPU fallback and no byte-checked path: what the one launch cannot serve is refused with
 * HGI_EUNSUPPORTED and the caller composes one hgi_typed_encode_dev call per view.
 */
#ifndef HGI_TVIEWS_H_
#define HGI_TVIEWS_H_

#include <stddef.h>
#include <stdint.h>

#include "hgi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One frame of a call.  Row y of the frame lies at src + y * src_pitch, `width` elements of elem_size    */
/* bytes; row y of the grid at dst + y * dst_pitch, `width` bytes.  The field offsets are hgi_view_pair's.*/
typedef struct hgi_tview_pair {
    uint64_t src, dst;             /* device addresses: the frame (elements), the grid (bytes) */
    uint32_t width, height;        /* pixels; a zero in either skips the entry */
    uint64_t src_pitch, dst_pitch; /* BYTES between rows on both sides (a one-row frame's pitch counts as its row) */
} hgi_tview_pair;

#define HGI_TVIEWS_MAGIC 0x56544731u /* "1GTV" */

/* What hgi_tviews_plan tells the launch about the blob it wrote (host memory, filled by the plan only):  */
/* hgi_views_info's layout with a magic of its own and the element size in the reserved slot.  The        */
/* quantizer table is host memory copied into the launch: nothing on the device to test against, so no    */
/* interval is recorded.                                                                                  */
typedef struct hgi_tviews_info {
    uint32_t magic;                /* HGI_TVIEWS_MAGIC */
    uint32_t count;                /* non-empty frames = records in the blob */
    uint32_t edge_tiles;           /* ragged 128 x 64 tiles over the list */
    uint32_t interior_tiles;       /* tiles whose body lies inside their frame */
    uint32_t max_width;            /* the widest frame, pixels */
    uint32_t elem_size;            /* bytes per input element the plan was made for: 2 or 4 (0: a plan of no entry) */
    uint64_t plan_bytes;           /* bytes of the blob in use: upload these */
    uint64_t records_offset;       /* count records of 64 bytes */
    uint64_t edge_prefix_offset;   /* count uint32: ragged tiles of the frames in front of each */
    uint64_t interior_prefix_offset; /* count uint32: interior tiles of the frames in front of each */
} hgi_tviews_info;

/* Bytes a plan of n entries needs at most (h_plan of hgi_tviews_plan; the upload is info->plan_bytes).   */
HGI_API size_t hgi_tviews_plan_bytes(size_t n);

/* ---- the plan: every argument rule of a list, decided on the host, without a HIP call ---------------- */
/*  - Writes the blob to h_plan (plan_bytes >= hgi_tviews_plan_bytes(n)) and fills *info.  On a refusal   */
/*    *info is all zero, the blob is untouched and no launch accepts the info.  n == 0: HGI_OK whatever   */
/*    the other arguments; only empty entries: HGI_OK, info->count == 0; a launch of such a plan succeeds */
/*    and does nothing.                                                                                   */
/*  - The blob holds addresses and sizes, no host pointer: copy it to the device (16-byte aligned) and    */
/*    keep it unchanged while launches that read it are in flight.  Device code never writes it.  A blob  */
/*    MODIFIED AFTER PLANNING IS UNDEFINED BEHAVIOUR: the launch validates `info`, not the device bytes.  */
/* HGI_EINVAL, decided before the HGI_EUNSUPPORTED rules, in this order (the text names the list index):  */
/*  - a NULL views, h_plan or info of a non-empty call; plan_bytes too small; elem_size not 2 or 4;       */
/*  - per non-empty entry, in list order: a NULL src or dst; a src that is no multiple of elem_size; and, */
/*    for a frame of more than one row, a src_pitch that is no multiple of elem_size, a src_pitch         */
/*    < width * elem_size, a dst_pitch < width;                                                           */
/*  - more tiles than a launch holds (the 128 x 64 tiles of all entries, padded, + 8 >= 2^31);            */
/*  - aliasing, on RECTANGLES OF BYTES exactly as in hgi_mviews.h, an input rectangle being               */
/*    width * elem_size bytes wide: frames may overlap each other; grids must be pairwise disjoint, and   */
/*    no grid may meet a frame.  Two rectangles whose byte spans meet are judged exactly when they have   */
/*    the same pitch or one of them is a single row; spans of two views of more than one row that meet    */
/*    with DIFFERENT pitches are refused, conservatively.                                                 */
/* HGI_EUNSUPPORTED (NOTHING written; compose one hgi_typed_encode_dev call per view):                    */
/*  - an entry whose offsets do not fit the 32-bit buffer path: with P the larger of its two BYTE         */
/*    pitches, P >= 2^32 or (height + 192) * P + 1024 >= 2^32;                                            */
/*  - the page rule of hgi_typed.h, per entry ON ITS OWN SPAN: elem_size 2, an odd width, and the two     */
/*    bytes behind the frame's span not in the 4-KiB page of the span's last byte: with end = src +       */
/*    (height - 1) * src_pitch + 2 * width the entry is served iff end is not a multiple of 4096.         */
/*    There is no page rule on the grid side: the grid is only written.                                   */
/* What a launch may READ beyond the width elements of the frame rows: gap elements inside a frame's span */
/* (any bit pattern, NaN and infinity included), and at elem_size 2 and an odd width the two bytes behind */
/* a view's last row.  Their values never influence a result.  The aliasing rule covers the width *      */
/* elem_size bytes of the frame rows only: another view's GRID of the same call may lie in a frame's gap  */
/* bytes or in those two tail bytes and be written while they are read; what is read there is then        */
/* indeterminate, and is masked or zeroed like any other gap value.                                       */
HGI_API hgi_status hgi_tviews_plan(const hgi_tview_pair *views, size_t n, uint32_t elem_size, void *h_plan, size_t plan_bytes,
                                   hgi_tviews_info *info);

/* ---- the launch -------------------------------------------------------------------------------------- */
/*  - Grid view i, read through its pitch, is bit for bit what hgi_encode_u8_dev makes of the packed      */
/*    uint8 image that hgi_typed.h's conversion makes of frame view i.  ONLY the `width` bytes of each    */
/*    grid row are written; the frames and the blob are never written.                                    */
/*  - elem_kind, scale, bias and lut belong to the launch, not to the view, and mean what they mean in    */
/*    hgi_typed.h: elem_kind 0 is IEEE (float16 at elem_size 2, float32 at 4), 1 is bfloat16 (elem_size 2 */
/*    only); `lut` is HOST memory, 256 bytes, copied into the launch; the identity table runs a           */
/*    residual-only instantiation.                                                                        */
/*  - Async on `hip_stream` (a hipStream_t; NULL = the default stream); the calling thread's current      */
/*    device must be the stream's.  d_plan: the device copy of the blob, 16-byte aligned.  Exactly ONE    */
/*    kernel launch for levels 1 ... 8 (up to five levels the 128 x 64 tile holds the pyramid; at six to  */
/*    eight the tile rebuilds the levels above it from its frame's own samples through the pitch).  No    */
/*    scratch; capturable into a graph.                                                                   */
/*  - A plan of no non-empty frame (info->count == 0, magic set): HGI_OK, nothing launched, decided first.*/
/* HGI_EINVAL, before the HGI_EUNSUPPORTED rule: a NULL info; an `info` that is inconsistent (magic,      */
/* elem_size, the sizes and offsets against the count, the block count); a NULL or misaligned d_plan; a   */
/* NULL lut; elem_kind > 1, or bfloat16 with a plan made for elem_size 4; a scale or bias that is not     */
/* finite; levels > 31; an unknown interpolator.  HGI_EUNSUPPORTED: levels == 0 or 9 <= levels <= 31.  A  */
/* failed launch returns HGI_EDEVICE.                                                                     */
HGI_API hgi_status hgi_tviews_encode_dev(void *hip_stream, const void *d_plan, const hgi_tviews_info *info, uint32_t elem_kind,
                                         float scale, float bias, uint32_t levels, hgi_interp interp, const uint8_t lut[256]);

/* Thread-local message of the calling thread's last failed hgi_tviews_* call (like hgi_last_error). */
HGI_API const char *hgi_tviews_last_error(void);

/* Library version; names the GPU architecture it was built for (gfx950). */
HGI_API const char *hgi_tviews_version(void);

#ifdef __cplusplus
}
#endif

#endif /* HGI_TVIEWS_H_ */
