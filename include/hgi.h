/*
 * hgi.h -- C ABI of the MI355X-native HGI encode/decode core (libhgi_hip.so).
 *
 * This is the drop-in boundary for the hot path of pl0q1n/RustyHGI: the
 * per-level grid interpolation + residual quantize loop.  The reference has no
 * FFI today; each entry point below names the reference interface it replaces
 * (paths relative to the reference repository).  INTEGRATION.md shows the
 * `extern "C"` block a maintainer adds on the Rust side.
 *
 * Conventions
 *  - plain pointers and sizes, no C++/torch types; never throws or aborts
 *    across the ABI: every call returns hgi_status, hgi_last_error() holds the
 *    thread-local message of the last failure;
 *  - images and grids are tightly packed row-major u8, stride == width
 *    (reference: GrayImage / Grid, src/grid.rs:2-27); a batch is `batch`
 *    frames `frame_stride` bytes apart.  The *_pitched calls alone take rows
 *    `pitch` >= width bytes apart, with a pitch and a frame stride of its own
 *    for the input and for the output (crops, canvas windows, padded planes);
 *    the region and scaled calls give their OUTPUT a pitch;
 *  - there is NO CPU fallback in this library: without a usable HIP device
 *    hgi_ctx_create fails with HGI_EDEVICE;
 *  - a ctx is not thread-safe; distinct ctxs are independent;
 *  - encode never modifies its input (the reference consumes it by value,
 *    src/encoder.rs:39);
 *  - `levels` in 0..=31 (1 << e on u32, src/utils.rs:17); levels == 0 makes
 *    grid == image; width or height == 0 is a successful no-op.
 */
#ifndef HGI_H_
#define HGI_H_

#include <stddef.h>
#include <stdint.h>

/* The shared object exports the entry points declared here and nothing else (built with        */
/* -fvisibility=hidden and a linker version script; tests/test_abi.py compares both directions). */
#if defined(__GNUC__) || defined(__clang__)
#define HGI_API __attribute__((visibility("default")))
#else
#define HGI_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hgi_ctx hgi_ctx;

/* src/interpolator.rs:15 (LeftTop), :30 (Crossed) -- the two implemented predictors */
typedef enum { HGI_INTERP_LEFTTOP = 0, HGI_INTERP_CROSSED = 1 } hgi_interp;

/* src/quantizator.rs:3-8 QuantizationLevel (bincode variant index) */
typedef enum {
    HGI_QUANT_LOSSLESS = 0,
    HGI_QUANT_LOW = 1,
    HGI_QUANT_MEDIUM = 2,
    HGI_QUANT_HIGH = 3
} hgi_quant_level;

typedef enum {
    HGI_OK = 0,
    HGI_EINVAL = 1,
    HGI_ENOMEM = 2,
    HGI_EDEVICE = 3,
    HGI_EUNSUPPORTED = 4
} hgi_status;

/* Which device implementation serves encode/decode (testing / benchmarking knob).   */
/* AUTO = FUSED.  Both run on the GPU; neither is a CPU path.                       */
typedef enum {
    HGI_PATH_AUTO = 0,
    HGI_PATH_LEVELWISE = 1, /* one launch per level, global-memory stencil            */
    HGI_PATH_FUSED = 2      /* all levels of a tile in one launch, LDS-resident       */
} hgi_path;

/* synthetic inputs of the harness; XY is benches/bench.rs:26-28 */
typedef enum { HGI_SYNTH_XY = 0, HGI_SYNTH_NOISE = 1, HGI_SYNTH_RAMP = 2 } hgi_synth_kind;

/* ---- context ---------------------------------------------------------------------- */
/* Owns the device id, a stream and scratch memory.  device >= 0 is a HIP ordinal.     */
HGI_API hgi_status hgi_ctx_create(int device, hgi_ctx **out);
HGI_API void hgi_ctx_destroy(hgi_ctx *ctx);
/* Borrow the caller's hipStream_t, used verbatim: NULL is HIP's default (null) stream,   */
/* which is what torch.cuda.current_stream() is unless a side stream is active.           */
HGI_API hgi_status hgi_ctx_set_stream(hgi_ctx *ctx, void *hip_stream);
/* Return to the ctx's private non-blocking stream (the state after hgi_ctx_create).      */
HGI_API hgi_status hgi_ctx_use_own_stream(hgi_ctx *ctx);
HGI_API hgi_status hgi_ctx_set_path(hgi_ctx *ctx, hgi_path path);
/* Pre-size scratch so later *_dev calls allocate nothing (needed before graph capture). */
/* Scratch only grows, and growing it FREES the old block: a HIP graph captured from calls */
/* that used scratch (pyramids deeper than eight levels; the level-wise path) keeps        */
/* pointing at the block it was captured with, so reserve for the largest shape the ctx    */
/* will ever see BEFORE capturing, and do not let a later, larger call on the same ctx     */
/* grow it while such graphs are alive.                                                    */
/* Covers hgi_encode_u8_dev / hgi_decode_u8_dev on `batch` frames of this shape AND the       */
/* host-pointer calls hgi_encode_u8 / hgi_decode_u8 on one such frame (their staging, the      */
/* seed planes of a banded deep pyramid); the host-pointer BATCH calls size their own slots.   */
HGI_API hgi_status hgi_ctx_reserve(hgi_ctx *ctx, uint32_t width, uint32_t height, uint32_t levels,
                           size_t batch);
/* Bytes of device scratch the ctx owns right now (0 after hgi_ctx_create): memory accounting,  */
/* and the way to see that a reserved ctx does not re-allocate.  Includes the frame lists'      */
/* descriptor tables and their pinned staging (hgi_*_u8_list_dev).                              */
HGI_API hgi_status hgi_ctx_scratch_bytes(hgi_ctx *ctx, size_t *bytes);
HGI_API hgi_status hgi_sync(hgi_ctx *ctx);
HGI_API const char *hgi_last_error(void);
HGI_API const char *hgi_version(void);

/* ---- quantizers (host side: any Quantizator is tabulated into 256 bytes) ----------- */
/* replaces Linear::from(QuantizationLevel) + Linear::error, src/quantizator.rs:41-63,71 */
HGI_API hgi_status hgi_linear_lut(int level, uint8_t lut[256], uint8_t *max_err);
/* replaces NoOp::quantize, src/quantizator.rs:26-29 */
HGI_API void hgi_noop_lut(uint8_t lut[256]);

/* ---- host-pointer, synchronous ------------------------------------------------------ */
/* replaces Encoder::<I,Q>::new(..).encode(image) -> Grid, src/encoder.rs:18,39          */
HGI_API hgi_status hgi_encode_u8(hgi_ctx *ctx, const uint8_t *img, uint32_t width, uint32_t height,
                         uint32_t levels, hgi_interp interp, const uint8_t lut[256],
                         uint8_t *grid_out);
/* replaces Decoder::<I>::new(..).decode((w,h), levels, &grid) -> GrayImage, src/decoder.rs:14,18 */
HGI_API hgi_status hgi_decode_u8(hgi_ctx *ctx, const uint8_t *grid, uint32_t width, uint32_t height,
                         uint32_t levels, hgi_interp interp, uint8_t *img_out);

/* ---- device-pointer, asynchronous on the ctx stream, batched -------------------------- */
/* Same semantics per frame; `lut` is a HOST pointer (256 bytes, copied into the launch).   */
/* frame_stride >= width*height; d_img / d_grid must not alias.                            */
HGI_API hgi_status hgi_encode_u8_dev(hgi_ctx *ctx, const void *d_img, uint32_t width, uint32_t height,
                             uint32_t levels, hgi_interp interp, const uint8_t lut[256],
                             void *d_grid, size_t batch, size_t frame_stride);
HGI_API hgi_status hgi_decode_u8_dev(hgi_ctx *ctx, const void *d_grid, uint32_t width, uint32_t height,
                             uint32_t levels, hgi_interp interp, void *d_img, size_t batch,
                             size_t frame_stride);

/* ---- region decode: a window of each frame, at a cost that follows the window ------------------ */
/* Decode the window [x0, x0 + region_width) x [y0, y0 + region_height) of each of `batch` frames.      */
/* Output pixel (i, j) of frame f = pixel (x0 + i, y0 + j) of hgi_decode_u8_dev's output, bit for bit.  */
/* Window row j of frame f goes to d_out + f * out_frame_stride + j * out_pitch, region_width bytes;     */
/* no other byte of d_out is written.  Async on the ctx stream.                                         */
/* Only the 128 x 64 tiles of the frame's tile lattice that intersect the window run;   */
/* pyramids of nine levels and more also decode the frame's stride-256 lattice first (w*h/65536 points) */
/* in scratch that hgi_ctx_reserve for the FRAME's shape covers; up to eight levels no scratch is used. */
/* Arguments (HGI_EINVAL unless noted):                                                                 */
/*  - the window lies inside the frame: x0 + region_width <= width, y0 + region_height <= height,       */
/*    computed in 64 bits;                                                                              */
/*  - out_pitch >= region_width; when batch > 1 also frame_stride >= width * height and                 */
/*    out_frame_stride >= (region_height - 1) * out_pitch + region_width;                               */
/*  - no aliasing, tested conservatively: the byte interval [d_out, d_out + (batch - 1) *               */
/*    out_frame_stride + (region_height - 1) * out_pitch + region_width) must not meet [d_grid,         */
/*    d_grid + (batch - 1) * frame_stride + width * height), even where the frames would interleave;    */
/*  - a zero-size window, batch == 0, width == 0 or height == 0 succeeds and writes nothing;            */
/*  - levels, interp and a NULL ctx as for hgi_decode_u8_dev; a ctx set to HGI_PATH_LEVELWISE:          */
/*    HGI_EUNSUPPORTED (region decode exists on the fused path only).                                   */
/* Any out_pitch, any alignment of d_out.                                                               */
HGI_API hgi_status hgi_decode_region_u8_dev(hgi_ctx *ctx, const void *d_grid, uint32_t width, uint32_t height,
                                            uint32_t levels, hgi_interp interp, uint32_t x0, uint32_t y0,
                                            uint32_t region_width, uint32_t region_height, void *d_out,
                                            size_t out_pitch, size_t batch, size_t frame_stride,
                                            size_t out_frame_stride);
/* One frame in host memory (pairs with hgi_decode_u8; what the CLI and the Python numpy path call).     */
/* Synchronous.  The whole grid is uploaded, only the window comes back: window row j goes to           */
/* out + j * out_pitch.  Same argument rules as above with batch = 1.                                   */
HGI_API hgi_status hgi_decode_region_u8(hgi_ctx *ctx, const uint8_t *grid, uint32_t width, uint32_t height,
                                        uint32_t levels, hgi_interp interp, uint32_t x0, uint32_t y0,
                                        uint32_t region_width, uint32_t region_height, uint8_t *out,
                                        size_t out_pitch);

/* ---- scaled decode: each frame at 1 / 2^shift resolution, from its coarse levels ------------------- */
/* Output frame f has sw = ceil(width / 2^shift) columns and sh = ceil(height / 2^shift) rows (computed */
/* in 64 bits).  Output pixel (i, j) = pixel (i << shift, j << shift) of hgi_decode_u8_dev's output,    */
/* bit for bit: the coarse levels of the pyramid are exact pixels of the image.  Row j  */
/* of frame f goes to d_out + f * out_frame_stride + j * out_pitch, sw bytes; no other byte of d_out is */
/* written.  Async on the ctx stream.  Only the grid bytes of the stride-2^shift lattice are read, and  */
/* levels - shift levels run on them; shift >= levels is a strided copy of the grid's own lattice.      */
/* Pyramids with nine levels and more left above the lattice also decode its stride-256 sub-lattice    */
/* first, in scratch that hgi_ctx_reserve for the FRAME's shape covers; up to eight none is used.       */
/* Arguments (HGI_EINVAL unless noted):                                                                 */
/*  - shift <= 31; out_pitch >= sw; when batch > 1 also frame_stride >= width * height and              */
/*    out_frame_stride >= (sh - 1) * out_pitch + sw;                                                    */
/*  - no aliasing, tested conservatively on byte spans as for region decode (the output span            */
/*    (batch - 1) * out_frame_stride + (sh - 1) * out_pitch + sw against the grid span);                */
/*  - batch == 0, width == 0 or height == 0 succeeds and writes nothing;                                */
/*  - levels, interp and a NULL ctx as for hgi_decode_u8_dev; a ctx set to HGI_PATH_LEVELWISE:          */
/*    HGI_EUNSUPPORTED (scaled decode exists on the fused path only).                                   */
/* Any out_pitch, any alignment of d_out.                                                               */
HGI_API hgi_status hgi_decode_scaled_u8_dev(hgi_ctx *ctx, const void *d_grid, uint32_t width, uint32_t height,
                                            uint32_t levels, hgi_interp interp, uint32_t shift, void *d_out,
                                            size_t out_pitch, size_t batch, size_t frame_stride, size_t out_frame_stride);
/* One frame in host memory.  Synchronous.  Only the sh grid rows the lattice lies on are uploaded      */
/* (gathered, one copy), only the sw x sh result comes back: row j goes to out + j * out_pitch.  Same   */
/* argument rules as above with batch = 1; hgi_ctx_reserve for the frame's shape covers its scratch.    */
HGI_API hgi_status hgi_decode_scaled_u8(hgi_ctx *ctx, const uint8_t *grid, uint32_t width, uint32_t height,
                                        uint32_t levels, hgi_interp interp, uint32_t shift, uint8_t *out, size_t out_pitch);

/* ---- pitched frames: rows `pitch` >= width bytes apart, a pitch of its own on each side ------------- */
/* A crop of a larger device image (d_img = parent + y0 * parent_width + x0, img_pitch = parent_width), a */
/* window of a canvas as decode target, planes with padded rows (hipMallocPitch, video surfaces): coded   */
/* where they lie, without a packing copy.  Row y of frame f lies at base + f * frame_stride + y * pitch,  */
/* `width` bytes.  Output frame f, read through its pitch, is bit for bit what hgi_encode_u8_dev /          */
/* hgi_decode_u8_dev write for the packed copy of input frame f.  Async on the ctx stream.                 */
/*  - ONLY the `width` bytes of each output row are written: the bytes between rows (pitch - width),       */
/*    between frames and around the span keep their values -- they may be a parent image's live pixels.    */
/*  - Reads stay inside each input frame's span [p, p + (height - 1) * pitch + width), plus at most three  */
/*    bytes behind the last frame's span when width is not a multiple of 4 and those bytes lie in the      */
/*    same 4-KiB page as the span's last byte (otherwise a byte-checked path runs).  Gap bytes inside the  */
/*    span may be read; their values never influence the result -- they are foreign data, not zeros, and   */
/*    corners beyond width / height read 0 whatever the gap holds.                                         */
/*  - Any pitch >= width, any alignment of base, pitch and frame stride; the two pitches are independent.  */
/*    Rows run on 16-B accesses whatever the width: a 1918-wide frame at pitch 2048 on a 128-B aligned     */
/*    base has every row start on a line boundary, which its packed form cannot have.      */
/*  - When both pitches equal `width` (and, batch > 1, both frame strides are one number) the call         */
/*    forwards to hgi_encode_u8_dev / hgi_decode_u8_dev: same kernels, tile order and tile heights.        */
/*    Otherwise 128 x 64 tiles in a simple walk (ragged tiles first, then row-major per frame).            */
/*  - Scratch: what hgi_ctx_reserve(width, height, levels, batch) covers; none up to eight levels.  From   */
/*    nine levels the stride-256 lattice is gathered through the pitch and coded in scratch first.         */
/*    Graph capture: as for the uniform _dev calls (reserve first; no table, no per-call device state).    */
/* Arguments (HGI_EINVAL unless noted):                                                                    */
/*  - a pitch < width; when batch > 1 a frame stride < (height - 1) * pitch + width of its side;           */
/*  - no aliasing, tested conservatively on byte spans as for region decode: [d_in, d_in + (batch - 1) *   */
/*    in_frame_stride + in_span) must not meet the output's interval -- two windows interleaved in one     */
/*    parent allocation (side by side in the same rows) are refused; windows of different allocations, or  */
/*    one above the other, are fine;                                                                       */
/*  - batch == 0, width == 0 or height == 0 succeeds and writes nothing;                                   */
/*  - levels, interp, lut and a NULL ctx as for the uniform calls; a ctx set to HGI_PATH_LEVELWISE:        */
/*    HGI_EUNSUPPORTED (pitched frames exist on the fused path only).                                      */
HGI_API hgi_status hgi_encode_u8_pitched_dev(hgi_ctx *ctx, const void *d_img, size_t img_pitch, uint32_t width,
                                             uint32_t height, uint32_t levels, hgi_interp interp,
                                             const uint8_t lut[256], void *d_grid, size_t grid_pitch, size_t batch,
                                             size_t img_frame_stride, size_t grid_frame_stride);
HGI_API hgi_status hgi_decode_u8_pitched_dev(hgi_ctx *ctx, const void *d_grid, size_t grid_pitch, uint32_t width,
                                             uint32_t height, uint32_t levels, hgi_interp interp, void *d_img,
                                             size_t img_pitch, size_t batch, size_t grid_frame_stride,
                                             size_t img_frame_stride);
/* One frame in host memory.  Synchronous.  Upload and download are 2-D copies of the width-byte rows     */
/* only (the gaps are neither read nor written; the last row goes on its own, so that no copy names a     */
/* byte behind the (height - 1) * pitch + width the array holds); between them the packed frame runs the  */
/* uniform route -- the host calls are transfer-bound.  Same argument rules as above with batch = 1;      */
/* hgi_ctx_reserve for the frame's shape covers the scratch.                                              */
HGI_API hgi_status hgi_encode_u8_pitched(hgi_ctx *ctx, const uint8_t *img, size_t img_pitch, uint32_t width,
                                         uint32_t height, uint32_t levels, hgi_interp interp,
                                         const uint8_t lut[256], uint8_t *grid_out, size_t grid_pitch);
HGI_API hgi_status hgi_decode_u8_pitched(hgi_ctx *ctx, const uint8_t *grid, size_t grid_pitch, uint32_t width,
                                         uint32_t height, uint32_t levels, hgi_interp interp, uint8_t *img_out,
                                         size_t img_pitch);

/* ---- frame lists: frames of different shapes in one call ------------------------------------------ */
/* Frame i is widths[i] x heights[i], tightly packed at d_imgs[i] / d_grids[i] (device pointers, any      */
/* alignment); its output is bit for bit what hgi_encode_u8_dev / hgi_decode_u8_dev write for that frame  */
/* alone.  Levels, interpolator and table are shared by the list (group by them in the caller).           */
/* The pointer and size arrays are HOST memory, read before the call returns: the caller may reuse or     */
/* free them at once.  `lut` as for hgi_encode_u8_dev.  Async on the ctx stream.                          */
/* Levels 1 ... 8 run as ONE launch over the 128 x 64 tiles of every frame; levels 0 and  */
/* from nine on are served frame by frame through the uniform calls (batch 1): correct, not batched.      */
/* The per-frame table goes up through a ring of ctx-owned slots (pinned staging + device table, both     */
/* grow-only, counted by hgi_ctx_scratch_bytes, freed by hgi_ctx_destroy); a call waits only for the      */
/* launch that last read the slot it reuses.  The scratch block is never touched by levels 1 ... 8.       */
/* Arguments (HGI_EINVAL unless noted):                                                                   */
/*  - count == 0 succeeds and does nothing; frames with width or height 0 are skipped (their pointers     */
/*    are not used);                                                                                      */
/*  - a NULL array with count > 0, or a NULL frame pointer of a non-empty frame, is refused;              */
/*  - overlaps, on byte spans [p, p + width * height): the outputs must be pairwise disjoint and no       */
/*    output may meet any input; inputs may overlap each other (one grid may be listed twice);            */
/*  - more tiles than one launch holds (2^31 - 16) is refused;                                            */
/*  - levels, interp and a NULL ctx as for hgi_decode_u8_dev; a ctx set to HGI_PATH_LEVELWISE, and a ctx  */
/*    stream that is being captured into a graph: HGI_EUNSUPPORTED (a replay would read a table that      */
/*    later calls overwrite).                                                                             */
HGI_API hgi_status hgi_encode_u8_list_dev(hgi_ctx *ctx, const void *const *d_imgs, const uint32_t *widths,
                                          const uint32_t *heights, uint32_t levels, hgi_interp interp,
                                          const uint8_t lut[256], void *const *d_grids, size_t count);
HGI_API hgi_status hgi_decode_u8_list_dev(hgi_ctx *ctx, const void *const *d_grids, const uint32_t *widths,
                                          const uint32_t *heights, uint32_t levels, hgi_interp interp,
                                          void *const *d_imgs, size_t count);

/* ---- host-pointer batch calls ------------------------------------------------------------ */
/* `batch` frames in HOST memory, frame f at base + f * frame_stride (frame_stride >= w*h). */
/* Synchronous like hgi_encode_u8 / hgi_decode_u8, but the frames are pipelined through the  */
/* device in chunks on two internal streams, so uploads overlap downloads (PCIe is full      */
/* duplex) and the kernels disappear behind the transfers.  Input and output must not alias. */
HGI_API hgi_status hgi_encode_u8_batch(hgi_ctx *ctx, const uint8_t *imgs, uint32_t width, uint32_t height,
                               uint32_t levels, hgi_interp interp, const uint8_t lut[256],
                               uint8_t *grids_out, size_t batch, size_t frame_stride);
HGI_API hgi_status hgi_decode_u8_batch(hgi_ctx *ctx, const uint8_t *grids, uint32_t width, uint32_t height,
                               uint32_t levels, hgi_interp interp, uint8_t *imgs_out, size_t batch,
                               size_t frame_stride);

/* ---- entropy front end (no counterpart in the reference, would precede the   */
/* DEFLATE of src/archive.rs:36) ---------------------------------------------------------- */
/* Byte histogram of each frame of a grid batch, on the device, async on the ctx stream:     */
/* d_hist[256*f + v] = number of pixels of frame f equal to v.  d_hist: 256*batch uint64 of  */
/* device memory (overwritten).  Any width, stride and alignment.                            */
HGI_API hgi_status hgi_histogram_u8_dev(hgi_ctx *ctx, const void *d_grid, uint32_t width, uint32_t height,
                                size_t batch, size_t frame_stride, void *d_hist);

/* ---- harness helpers (not part of the reference surface) ------------------------------ */
/* Fill `batch` frames with a synthetic pattern; frame f uses index first_frame + f.        */
HGI_API hgi_status hgi_synth_u8_dev(hgi_ctx *ctx, hgi_synth_kind kind, uint64_t seed,
                            uint64_t first_frame, uint32_t width, uint32_t height, void *d_out,
                            size_t batch, size_t frame_stride);
/* Streaming copy of n bytes (16-B vectors): the same-run HBM copy ceiling.                 */
HGI_API hgi_status hgi_copy_u8_dev(hgi_ctx *ctx, const void *d_src, void *d_dst, size_t n);
/* Per-frame statistics of before/after pairs as `hgi test` prints them (src/main.rs:84-92): */
/* out[3*f+0] = sum of squared differences, +1 = max abs difference, +2 = count of differing */
/* pixels.  d_out is device memory for 3*batch uint64.                                       */
HGI_API hgi_status hgi_diff_stats_dev(hgi_ctx *ctx, const void *d_before, const void *d_after,
                              uint32_t width, uint32_t height, size_t batch, size_t frame_stride,
                              void *d_out);
/* ---- entropy stage on the device (the step behind src/archive.rs:34-40) ------------------- */
/* Raw DEFLATE (RFC 1951: one dynamic-Huffman block of literals and run matches -- a byte that */
/* repeats its predecessor is covered by matches of distance 1) of the bincode image of a Grid */
/* -- u64 w*h, the w*h residual bytes at d_grid, u64 w -- i.e. exactly the bytes that follow   */
/* the metadata in a .hgi archive.  Tokens, histogram, bit counting, scan and bit packing run  */
/* on the device; the 286-symbol code and the block header are built on the host.  Any inflate */
/* reads the result (the reference's flate2 DeflateDecoder included).  Residual grids are      */
/* noise around zero, in which LZ77 finds runs and nothing else: the stream is within a few %  */
/* of DEFLATE at the best level on smooth images and smaller than it on busy ones (LENA /      */
/* Medium: 14.0 against 16.0 kB) -- and written two to four orders of magnitude sooner.        */
/* `out` is host memory; *bytes receives the stream length; HGI_EINVAL if cap is too small     */
/* (w*h + w*h/8 + 1024 always suffices).  Synchronous on the ctx stream.                        */
HGI_API hgi_status hgi_deflate_grid_dev(hgi_ctx *ctx, const void *d_grid, uint32_t width, uint32_t height,
                                uint8_t *out, size_t cap, size_t *bytes);
/* `batch` grids `frame_stride` bytes apart in device memory: stream f is written to            */
/* out + f * out_stride (host memory; out_stride is also each stream's capacity), sizes[f] = its */
/* length.  The batch is pipelined in groups of frames (256 MiB of stream buffer each): one    */
/* launch per phase per group, the host building a group's codes while the device histograms   */
/* the next, a group's streams going down while the next is coded.  The downloads bound the    */
/* call; they are faster into pinned host memory (a 1 GiB batch: 5.5 ms pageable, 4.5 pinned). */
/* `out` is written from a second stream internally; the call returns when everything is done. */
HGI_API hgi_status hgi_deflate_grids_dev(hgi_ctx *ctx, const void *d_grids, uint32_t width, uint32_t height, size_t batch,
                                 size_t frame_stride, uint8_t *out, size_t out_stride, size_t *sizes);
/* The same batch with the streams PACKED into one host buffer of `cap` bytes: stream f occupies */
/* out[offsets[f] .. offsets[f] + sizes[f]), offsets ascending and multiples of 64.  The sizes are */
/* known from the histograms before anything is packed, so a group's streams lie back to back on  */
/* the device and come down with ONE copy per group instead of one per frame (each copy costs a   */
/* fixed ~12 us on top of its bytes).  The gap between a stream's end and the next stream's start  */
/* (at most 63 bytes) is zero.  HGI_EINVAL when `cap` does not hold them all                       */
/* (batch * (w*h + w*h/8 + 1088) always suffices).                                                  */
HGI_API hgi_status hgi_deflate_grids_packed_dev(hgi_ctx *ctx, const void *d_grids, uint32_t width, uint32_t height, size_t batch,
                                                size_t frame_stride, uint8_t *out, size_t cap, size_t *offsets, size_t *sizes);
/* The same with the grid in host memory (what pairs with hgi_encode_u8).                      */
HGI_API hgi_status hgi_deflate_grid(hgi_ctx *ctx, const uint8_t *grid, uint32_t width, uint32_t height,
                            uint8_t *out, size_t cap, size_t *bytes);
/* The code construction alone (host only): lengths (<= 15) and bit-reversed canonical codes    */
/* of the 286 symbols -- literals 0..255, end of block 256 (hist[256]), match lengths 257..285 */
/* -- for the given counts, and the block header (BFINAL = 1, dynamic, 286 + 2 codes; distance */
/* code 0 = distance 1 is the one-bit code "0") that announces them; *header_bits = its length.*/
HGI_API hgi_status hgi_huffman_plan(const uint64_t hist[286], uint8_t lens[286], uint16_t codes[286],
                            uint8_t *header, size_t header_cap, size_t *header_bits);

/* ---- plane placement (no reference counterpart: the reference's buffers are Vec<u8>) ---- */
/* MI355X's HBM falls into a few classes of physical memory; a launch that streams one buffer */
/* in and another out runs 4-8 % faster when the two lie in different classes. */
/* hgi_planes_alloc returns `count` device buffers of at least `bytes` each such that          */
/* planes[i] and planes[i+1] lie in different classes over their whole length: image -> grid   */
/* -> image chains alternate through the array.  RELEASE THEM WITH hgi_planes_free ONLY.       */
/* Best effort, found by timing a decode launch between candidates against a same-class        */
/* yardstick; *separated (optional) is 1 when every neighbouring pair was seen to stream at    */
/* the fast rate, 0 when that could not be established -- the planes are valid either way.     */
/*  - planes below 128 MiB: plain hipMalloc, not probed (such streams live in the 256 MiB      */
/*    Infinity Cache);                                                                         */
/*  - 128 MiB up to 1 GiB: allocated at 1 GiB each so that the probe can tell (a launch over   */
/*    two of them no longer fits that cache: a lone 16384 x 16384 frame gains 2-3 %); if the   */
/*    device lacks the memory for that they come back at `bytes`, unplaced;                    */
/*  - exactly 1 GiB: whole hipMalloc allocations are the candidates (typically 30-50 ms; up   */
/*    to ten extra candidates and spacers when the first ones share a class);                  */
/*  - above 1 GiB: each plane is one reserved address range onto which physical chunks of      */
/*    1 GiB (hipMemCreate) are mapped, chosen chunk by chunk (size rounded up to whole GiB).   */
/*    Bounded: at most 3 x the requested bytes are ever created as candidates, plus at most    */
/*    96 GiB of never-mapped spacers when the driver keeps handing out one class; what is not  */
/*    handed out is released before the call returns (three planes of 8 GiB: 1-2 s).           */
/* HGI_NO_PLACEMENT=1 in the environment skips all of it (plain allocations): the one variable */
/* the library reads.  Call it while the device is otherwise idle: it measures.                */
HGI_API hgi_status hgi_planes_alloc(hgi_ctx *ctx, size_t bytes, uint32_t count, void **planes, int *separated);
/* One line on what the last hgi_planes_alloc of this ctx found and did -- candidates created,   */
/* how many share which class, which line-up the planes got -- for logs and bench records (how   */
/* fast a large encode runs follows it).  Owned by the ctx, overwritten by its    */
/* next hgi_planes_alloc; "" before the first.                                                   */
HGI_API const char *hgi_planes_report(hgi_ctx *ctx);
HGI_API hgi_status hgi_planes_free(hgi_ctx *ctx, uint32_t count, void **planes);
/* The probe itself: mean milliseconds of one decode launch streaming d_src -> d_dst over      */
/* min(bytes, 2 GiB).  Overwrites d_dst.  Compare pairings of the caller's own buffers with it. */
HGI_API hgi_status hgi_probe_pair_u8_dev(hgi_ctx *ctx, const void *d_src, void *d_dst, size_t bytes, float *ms);

/* hipEvent pair on the ctx stream: start, ...launches..., stop -> elapsed milliseconds.     */
HGI_API hgi_status hgi_timer_start(hgi_ctx *ctx);
HGI_API hgi_status hgi_timer_stop(hgi_ctx *ctx, float *elapsed_ms);

#ifdef __cplusplus
}
#endif
#endif /* HGI_H_ */
