/*
 * hgi_qviews.h -- C ABI of libhgi_qviews.so: requantize view lists, mixed-size grids re-coded with
 * another quantizer in ONE launch on the MI355X.
 *
 * A companion of libhgi_hip.so (hgi.h).  hgi_requant.h re-codes stored grids with another table at
 * 2 B/px, but one shape and one pitch pair per call; hgi_views.h codes lists of views that each bring a
 * shape and two pitches of their own, but a list goes from grids to grids only through a uint8 image
 * nobody wants: two launches and 4 B/px.  Here a list of stored grids of different sizes -- an archive
 * tier going Lossless to Medium, a thumbnail store going Medium to High -- is re-coded in one launch.
 *
 * THE PLAN IS hgi_views_plan's (hgi_views.h), unchanged: `src` of an entry is the grid that is READ,
 * `dst` the grid that is WRITTEN.  Every rule requantize needs is a rule of that plan: the page rule per
 * entry on the source span, the 32-bit bound over both pitches, outputs pairwise disjoint, no output
 * meeting an input -- IN PLACE IS REFUSED with that, as hgi_requant.h refuses it -- and inputs free to
 * overlap.  A blob and an info a caller already holds serve here as they stand; this library has no
 * plan entry, no blob, no record and no magic of its own.
 *
 * This header takes hgi_status and hgi_interp from hgi.h and hgi_views_info from hgi_views.h; the
 * library links nothing of libhgi_hip.so and nothing of libhgi_views.so, keeps no state (no ctx, no
 * scratch, no device allocation) and reads no environment variable.  There is NO CPU fallback and no
 * byte-checked path: what the one launch cannot serve is refused with HGI_EUNSUPPORTED and the caller
 * composes one hgi_requant_dev call per view.
 */
#ifndef HGI_QVIEWS_H_
#define HGI_QVIEWS_H_

#include <stddef.h>
#include <stdint.h>

#include "hgi.h"
#include "hgi_views.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the launch -------------------------------------------------------------------------------------- */
/*  - d_plan: the device copy of a blob written by hgi_views_plan, 16-byte aligned; info: the host struct */
/*    that plan filled (HGI_VIEWS_MAGIC).  The infos of the mapped and the typed view lists are refused.  */
/*  - Destination view i, read through its pitch, is bit for bit                                          */
/*        hgi_encode_u8_dev(hgi_decode_u8_dev(src_i, levels, interp), levels, interp, lut)                */
/*    on the packed copy of source view i alone.  ONE `levels`, ONE `interp` and ONE table serve the      */
/*    whole list and both directions (a change of depth or predictor stays a composition by the caller).  */
/*  - ONLY the `width` bytes of each destination row are written.  Sources and the blob are never         */
/*    written.  What may be READ beyond the `width` bytes of the source rows is what hgi_views.h states.  */
/*  - Async on `hip_stream` (a hipStream_t; NULL = the default stream); the calling thread's current      */
/*    device must be the stream's.  `lut` is HOST memory, 256 bytes, copied into the launch: the caller   */
/*    may reuse it at once.                                                                               */
/*  - Exactly ONE kernel launch for levels 1 ... 8: up to five levels the 128 x 64 tile holds the         */
/*    pyramid, at six to eight the tile rebuilds the levels above it from its source grid through the     */
/*    pitch (the cone), once in each direction.  No scratch, no state; capturable into a graph.           */
/*  - A plan of no non-empty entry (info->count == 0, magic set): HGI_OK, nothing launched.  That is      */
/*    decided first, whatever the other arguments are.                                                    */
/* HGI_EINVAL, in this order, all before the HGI_EUNSUPPORTED rules:                                      */
/*  - a NULL info;                                                                                        */
/*  - an `info` that is inconsistent (magic, the sizes and offsets against the count, the block count);   */
/*  - a NULL d_plan; a d_plan that is not 16-byte aligned;                                                */
/*  - a NULL lut;                                                                                         */
/*  - levels > 31;                                                                                        */
/*  - an interp other than the two of hgi_interp.                                                         */
/* HGI_EUNSUPPORTED, in this order (message in hgi_qviews_last_error(), NOTHING written):                 */
/*  - levels == 0 or 9 <= levels <= 31 (compose one hgi_requant_dev call per view, which composes decode  */
/*    + encode in turn);                                                                                  */
/*  - the identity table (lut[i] == i for all i).  Under it the encoder keeps every residual, so encoding */
/*    a decoded grid gives the grid back: the result IS the source.  Copy the source instead; no kernel   */
/*    is built for this table.                                                                            */
/* Every rule is decided before the first HIP call.  A failed launch returns HGI_EDEVICE.                 */
HGI_API hgi_status hgi_qviews_requant_dev(void *hip_stream, const void *d_plan, const hgi_views_info *info, uint32_t levels,
                                          hgi_interp interp, const uint8_t lut[256]);

/* Thread-local message of the calling thread's last failed hgi_qviews_* call (like hgi_last_error). */
HGI_API const char *hgi_qviews_last_error(void);

/* Library version; names the GPU architecture it was built for (gfx950). */
HGI_API const char *hgi_qviews_version(void);

#ifdef __cplusplus
}
#endif

#endif /* HGI_QVIEWS_H_ */
