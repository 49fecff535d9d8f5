/*
 * hgi_rviews.h -- C ABI of libhgi_rviews.so: recon view lists, frames of different shapes encoded into
 * grids AND into the images the decoder will make of those grids, every frame with a pitch of its own on
 * each of its three sides, in ONE launch on the MI355X.
 *
 * A companion of libhgi_hip.so (hgi.h).  Encode with reconstruction (hgi_recon.h) writes the grid and the
 * reconstruction from one launch at 3 B/px, but one shape and one pitch set per call; the view lists
 * (hgi_views.h) code frames of different shapes in one launch, but two-sided: grid and reconstruction of
 * a list are hgi_views_encode_dev + hgi_views_decode_dev, two launches at 4 B/px.  Here every frame of a
 * call brings {pointer, row pitch} for the image that is read, for the grid that is written and for the
 * reconstruction that is written, and its size: the sprites of an atlas, the tiles of a mosaic, a ragged
 * thumbnail store inside a rate/quality search or a difference coder.
 *
 * PLAN ONCE, LAUNCH MANY, as in hgi_views.h: hgi_rviews_plan is pure host code, judges every rule of the
 * list and writes a position-independent blob into caller memory and a small host struct; the caller
 * uploads the blob and hands its device address to any number of launches.  A launch is exactly one
 * kernel launch with nothing else on the stream: stateless and capturable into a graph.  The plan depends
 * on neither the depth, the interpolator nor the table.
 *
 * This header takes hgi_status and hgi_interp from hgi.h; the library links nothing of libhgi_hip.so,
 * keeps no state (no ctx, no scratch, no device allocation) and reads no environment variable.  There is
 * NO CPU fallback and no byte-checked path: what the one launch cannot serve is refused with
 * HGI_EUNSUPPORTED and the caller composes one hgi_recon_encode_u8_dev call per view.
 */
#ifndef HGI_RVIEWS_H_
#define HGI_RVIEWS_H_

#include <stddef.h>
#include <stdint.h>

#include "hgi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One frame of a call.  Row y lies at base + y * pitch, `width` bytes, on each of its three sides.      */
typedef struct hgi_rview_triple {
    uint64_t src, grid, recon;     /* device addresses: image read, grid written, reconstruction written */
    uint32_t width, height;        /* pixels; a zero in either skips the entry */
    uint64_t src_pitch, grid_pitch, recon_pitch; /* bytes between rows, >= width (a one-row frame's pitch counts as its width) */
} hgi_rview_triple;

#define HGI_RVIEWS_MAGIC 0x56524731u /* "1GRV" */

/* What hgi_rviews_plan tells the launch about the blob it wrote (host memory, filled by the plan only):  */
/* hgi_views_info's layout with a magic of its own, and where the third side's records stand.             */
typedef struct hgi_rviews_info {
    uint32_t magic;                /* HGI_RVIEWS_MAGIC */
    uint32_t count;                /* non-empty frames = records in the blob */
    uint32_t edge_tiles;           /* ragged 128 x 64 tiles over the list */
    uint32_t interior_tiles;       /* tiles whose body lies inside their frame */
    uint32_t max_width;            /* the widest frame */
    uint32_t reserved;             /* 0 */
    uint64_t plan_bytes;           /* bytes of the blob in use: upload these */
    uint64_t records_offset;       /* count records of 64 bytes: the (src, grid) pairs, as hgi_views_plan writes them */
    uint64_t edge_prefix_offset;   /* count uint32: ragged tiles of the frames in front of each */
    uint64_t interior_prefix_offset; /* count uint32: interior tiles of the frames in front of each */
    uint64_t recon_offset;         /* count records of 16 bytes: {uint64 recon; uint32 pitch; uint32 span} */
} hgi_rviews_info;

/* Bytes a plan of n entries needs at most (h_plan of hgi_rviews_plan; the upload is info->plan_bytes).   */
HGI_API size_t hgi_rviews_plan_bytes(size_t n);

/* ---- the plan: every argument rule of a list, decided on the host, without a HIP call ---------------- */
/*  - Writes the blob to h_plan (plan_bytes >= hgi_rviews_plan_bytes(n)) and fills *info.  On a refusal   */
/*    NOTHING is written to h_plan, info->magic is 0 and no launch accepts the info.  n == 0 or only      */
/*    empty entries: HGI_OK, info->count == 0, and a launch of that plan succeeds and does nothing.       */
/*  - The blob holds addresses and sizes, no host pointer: copy it to the device (16-byte aligned) and    */
/*    keep it unchanged while launches that read it are in flight.  Device code never writes it.  A blob  */
/*    MODIFIED AFTER PLANNING IS UNDEFINED BEHAVIOUR: the launch validates `info`, not the device bytes.  */
/*  - The blob's first bytes, up to recon_offset, are byte for byte the blob hgi_views_plan writes for    */
/*    the (src, grid) pairs of the list; behind them stands one 16-byte record per non-empty frame: the   */
/*    reconstruction's address, its 32-bit pitch and its span (height - 1) * pitch + width.               */
/* HGI_EINVAL, decided before the HGI_EUNSUPPORTED rules, in this order (the text names the list index):  */
/*  - a NULL triples, h_plan or info of a non-empty call; plan_bytes too small;                           */
/*  - per non-empty entry, in list order: a NULL src, grid or recon; then src_pitch, grid_pitch or        */
/*    recon_pitch < width where height > 1 (a one-row frame's pitches are not looked at);                 */
/*  - more tiles than a launch holds: the 128 x 64 tiles of all entries, padded, + 8 >= 2^31.  Tiles are  */
/*    counted ONCE per entry: one tile writes both outputs;                                               */
/*  - aliasing, on RECTANGLES OF BYTES exactly as in hgi_views.h, with three rectangles per entry, each   */
/*    width x height at its side's pitch.  Inputs may overlap each other (two crops of one image).  All   */
/*    2 * count outputs, grids and reconstructions alike, must be pairwise disjoint, and no output may    */
/*    meet an input -- in place is refused with that: a tile's halo reads its neighbours' originals.      */
/*    Rectangles whose byte spans [p, p + (height - 1) * pitch + width) do not meet are fine.  Two whose  */
/*    spans meet are judged exactly when both have the same pitch P: with the lower address as origin the */
/*    other one starts at column (b - a) mod P, row (b - a) / P; the pair is fine iff that column plus    */
/*    its width is <= P and the two rectangles are disjoint (a grid window and a reconstruction window    */
/*    side by side in one parent's rows).  A one-row rectangle is an interval of bytes and is judged      */
/*    exactly against any other.  Spans of two rectangles of more than one row that meet with DIFFERENT   */
/*    pitches are refused, conservatively.  The text names the list index and the side (grid or           */
/*    reconstruction) of each rectangle of the offending pair.                                            */
/* HGI_EUNSUPPORTED (NOTHING written; compose one hgi_recon_encode_u8_dev call per view):                 */
/*  - an entry whose offsets do not fit the 32-bit buffer path: with P the largest of its THREE pitches   */
/*    (a one-row frame's pitch counts as its width), P >= 2^32 or (height + 192) * P + 1024 >= 2^32;      */
/*  - an entry with width % 4 != 0 whose three bytes behind ITS OWN source span leave the 4-KiB page of   */
/*    the span's last byte: with end = src + (height - 1) * src_pitch + width the entry is served iff     */
/*    (end - 1) >> 12 == (end + 2) >> 12.  The outputs have no page rule: nothing is read from them.      */
/* What a launch may READ beyond the width bytes of the source rows: gap bytes inside a source span, and  */
/* at most three bytes behind a view's last row when its width is not a multiple of 4.  Their values      */
/* never influence a result, even if another view of the same call is writing them.                      */
HGI_API hgi_status hgi_rviews_plan(const hgi_rview_triple *triples, size_t n, void *h_plan, size_t plan_bytes, hgi_rviews_info *info);

/* ---- the launch -------------------------------------------------------------------------------------- */
/*  - Grid view i, read through its pitch, is bit for bit what hgi_encode_u8_dev writes for the packed    */
/*    copy of source view i alone; recon view i is bit for bit what hgi_decode_u8_dev writes for that     */
/*    grid.  ONLY the `width` bytes of each output row are written, on both outputs; the sources and the  */
/*    blob are never written.  One `levels`, one `interp` and one table serve the whole list.             */
/*  - Async on `hip_stream` (a hipStream_t; NULL = the default stream); the calling thread's current      */
/*    device must be the stream's.  `lut` is HOST memory, 256 bytes, copied into the launch.  The         */
/*    identity table (lut[i] == i) runs a residual-only instantiation in the same launch and writes the   */
/*    image's own bytes as the reconstruction, as in hgi_recon.h.  d_plan: the device copy of the blob,   */
/*    16-byte aligned.  Exactly ONE kernel launch for levels 1 ... 8 (up to five levels the 128 x 64 tile */
/*    holds the pyramid; at six to eight the tile rebuilds the levels above it from its frame's own       */
/*    samples through the pitch: the cone).  No scratch, no state; capturable into a graph.               */
/*  - A plan of no non-empty frame (info->count == 0, magic set): HGI_OK, nothing launched, decided first.*/
/* HGI_EINVAL, before the HGI_EUNSUPPORTED rule, in this order: a NULL info; an `info` that is            */
/* inconsistent (the magic -- the infos of hgi_views.h, hgi_mviews.h, hgi_tviews.h and hgi_sviews.h are   */
/* refused here --, the sizes and offsets against the count, recon_offset among them, the block count);   */
/* a NULL d_plan, or one that is not 16-byte aligned; a NULL lut; levels > 31; an unknown interpolator.   */
/* HGI_EUNSUPPORTED: levels == 0 or 9 <= levels <= 31.  A failed launch returns HGI_EDEVICE.              */
HGI_API hgi_status hgi_rviews_encode_dev(void *hip_stream, const void *d_plan, const hgi_rviews_info *info, uint32_t levels,
                                         hgi_interp interp, const uint8_t *lut);

/* Thread-local message of the calling thread's last failed hgi_rviews_* call (like hgi_last_error). */
HGI_API const char *hgi_rviews_last_error(void);

/* Library version; names the GPU architecture it was built for (gfx950). */
HGI_API const char *hgi_rviews_version(void);

#ifdef __cplusplus
}
#endif

#endif /* HGI_RVIEWS_H_ */
