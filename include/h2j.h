/*
 * h2j.h — C ABI of libH265ToJpeg.so beyond the reference's C++ surface.
 *
 * The reference exports exactly two entry points for this path
 * (SURVEY.md §8b):
 *   - IDecoder::getInstance() / virtual bool H265ToJpeg(in, out)
 *       (/root/reference/export_inc/IDecoder.h:29,35)       -> include/IDecoder.h
 *   - Java_com_autonavi_socol_occtiltedserver_service_H265DecodeService_decode
 *       (/root/reference/src/jni/com_autonavi_socol_occtiltedserver_service_H265DecodeService.h:15-16)
 * Both are kept verbatim.  The functions below are the batch engine those
 * entry points sit on; they are what an FFI binding (ctypes, cgo, N-API)
 * would bind for throughput, see INTEGRATION.md.
 *
 * Return values: 0 success, < 0 error (message via h2j_engine_error).
 *
 * Input: wherever a call takes the bytes of a stream (data / sizes), they are an Annex-B elementary
 * stream of either codec, or a HEIF / HEIC file (DESIGN.md "HEIF input"): its primary item, a single
 * hvc1 / avc1 item or a grid of hvc1 tiles decoded as one picture of the grid's output size.  A HEIF
 * file that cannot be read fails alone with a status in -110..-115 and its own frame-error message.
 * Its irot / imir properties stand where a stream's display orientation SEI stands (H2J_ORIENT_AUTO,
 * h2j_stream_orientation): never applied unasked.
 */
#ifndef H2J_H
#define H2J_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct h2j_engine h2j_engine;

/* Visible HIP devices (0: the MI355X pipeline cannot run). */
int h2j_device_count(void);

/* device: HIP device ordinal; host_threads: entropy/Huffman threads (the caller's thread
 * included).  > 0: exactly that many.  0: automatic -- the process's CPUs on the device's NUMA
 * node, split between the visible devices of that node, bounded by the cgroup CPU quota and 64;
 * the pool's workers are pinned to that NUMA-local slice (H2J_PIN=0: not pinned).  -k: as 0,
 * for one of k engines in this process (they share the cgroup quota). */
h2j_engine *h2j_engine_create(int device, int host_threads);
void h2j_engine_destroy(h2j_engine *e);
const char *h2j_engine_error(h2j_engine *e);
/* Message of picture i of the last h2j_engine_transcode ("" if it succeeded).  The string stays
 * valid until the calling thread's next h2j_engine_frame_error call. */
const char *h2j_engine_frame_error(h2j_engine *e, int i);
/* Host placement: out[0] threads (incl. the caller), [1] the device's NUMA node (-1 unknown),
 * [2] CPUs the workers are pinned to (0: not pinned), [3] first of those CPUs. */
int h2j_engine_host_info(h2j_engine *e, int *out, int n);

/* Transcode n independent Annex-B stills (H.264 or H.265, first picture of
 * each) to baseline JPEG.  JPEG i is written at out + out_off[i], length
 * out_len[i]; status[i] = 0 on success, < 0 on failure for that item.
 * Returns 0 if the batch ran (per-item failures reported in status), < 0
 * if the batch could not run (e.g. no GPU, out_cap too small). */
int h2j_engine_transcode(h2j_engine *e, int n, const uint8_t *const *data, const size_t *sizes,
                         uint8_t *out, size_t out_cap, size_t *out_off, size_t *out_len, int *status);

/* Asynchronous batches.  h2j_engine_submit queues a batch (same arguments and per-item
 * semantics as h2j_engine_transcode) and returns a ticket (> 0) at once; the engine parses
 * batches in submission order on its thread pool and runs their GPU work and JPEG assembly on a
 * driver thread, so one batch's GPU tail overlaps the next batch's entropy decoding.  A
 * submitted batch is cut into chunks of up to 1024 pictures (K1 then reconstructs up to four
 * pictures per workgroup).  Every pointer passed to submit must stay valid until
 * h2j_engine_wait returns for that ticket; h2j_engine_wait returns what h2j_engine_transcode
 * would have.  h2j_engine_transcode is submit + wait with smaller, latency-oriented chunks.
 * Stats, chunk times and frame errors describe the last batch that finished. */
int64_t h2j_engine_submit(h2j_engine *e, int n, const uint8_t *const *data, const size_t *sizes,
                          uint8_t *out, size_t out_cap, size_t *out_off, size_t *out_len, int *status);
int h2j_engine_wait(h2j_engine *e, int64_t ticket);

/* Scaled output (no counterpart in the reference, whose Encoder always encodes the decoded
 * size): the JPEG of a picture at 1/2, 1/4 or 1/8 of its decoded size, made on the GPU by a box
 * filter (DESIGN.md "Scaled output" has the exact arithmetic).  For a W x H picture at scale k
 * the JPEG is W_k x H_k with W_k = 2 ceil(W / 2^(k+1)), H_k = 2 ceil(H / 2^(k+1)); k = 0 is the
 * unscaled output, byte for byte. */
typedef struct {
    int32_t scale_log2; /* 0..3: output at 1/1, 1/2, 1/4, 1/8 */
    int32_t max_dim;    /* 0: off.  > 0: the smallest k in [scale_log2, 3] with
                           max(W_k, H_k) <= max_dim; 3 if none fits */
} h2j_out_opts;
/* status of an item whose options are invalid (scale_log2 outside 0..3, max_dim < 0); the item
 * fails alone, with a h2j_engine_frame_error message */
#define H2J_ERR_OUT_OPTS (-60)

/* h2j_engine_submit / h2j_engine_transcode with per-item output options: opts has n entries
 * (copied by the call), NULL = all {0, 0}, which is exactly the calls above.  The same stream
 * may appear several times with different options (the full picture and a thumbnail in one
 * batch); every item is parsed on its own (h2j_engine_transcode_multi below parses a picture once
 * for all of its outputs). */
int64_t h2j_engine_submit_opts(h2j_engine *e, int n, const uint8_t *const *data, const size_t *sizes,
                               const h2j_out_opts *opts, uint8_t *out, size_t out_cap, size_t *out_off,
                               size_t *out_len, int *status);
int h2j_engine_transcode_opts(h2j_engine *e, int n, const uint8_t *const *data, const size_t *sizes,
                              const h2j_out_opts *opts, uint8_t *out, size_t out_cap, size_t *out_off,
                              size_t *out_len, int *status);

/* Exact-size output: the JPEG of a picture at a size the caller names, made on the GPU by an
 * area-average resampler (DESIGN.md "Exact-size output (K3r)" has the exact arithmetic).
 * fit_w x fit_h is a box the output fits inside with the picture's aspect kept, or, with
 * H2J_FIT_STRETCH, the output size itself; a 0 leaves that axis unbounded.  The output never
 * upscales and is always even (h2j_fit_size below is the rule).  A box no smaller than the
 * picture gives the unscaled output, byte for byte; a size that is the picture's at 1/2, 1/4 or
 * 1/8 gives the bytes of that scale_log2. */
#define H2J_FIT_STRETCH 1
typedef struct {
    int32_t scale_log2, max_dim; /* as h2j_out_opts */
    int32_t fit_w, fit_h;        /* 0: no bound on that axis; else 2..65535 */
    int32_t flags;               /* H2J_FIT_STRETCH = 1 */
    int32_t reserved[3];         /* must be 0 */
} h2j_out_opts2;
/* Invalid (the item fails alone with H2J_ERR_OUT_OPTS): what is invalid in h2j_out_opts; fit_w or
 * fit_h negative, 1 or above 65535; unknown flag bits or non-zero reserved; a fit field together
 * with scale_log2 != 0 or max_dim != 0; H2J_FIT_STRETCH with both fit fields 0. */

/* The size rule, a pure function (no engine, no GPU): the output size *ow x *oh of a cropped
 * w x h picture (both even, 2..8192) for fit_w, fit_h, flags as in h2j_out_opts2.  With
 * bw = fit_w ? min(fit_w, w) : w and bh likewise: fit inside, the width binds when
 * bw * h <= bh * w: ow = 2 (bw / 2), oh = 2 max(1, (h * ow) / (2 w)); else the height binds,
 * symmetrically; stretch: ow = 2 (bw / 2), oh = 2 (bh / 2).  All divisions floor.
 * Returns 0, or H2J_ERR_OUT_OPTS for invalid arguments (ow, oh are not written). */
int h2j_fit_size(int w, int h, int fit_w, int fit_h, int flags, int *ow, int *oh);

/* h2j_engine_submit_opts / h2j_engine_transcode_opts with h2j_out_opts2; an h2j_out_opts item
 * is the h2j_out_opts2 item with fit_w = fit_h = flags = 0. */
int64_t h2j_engine_submit_opts2(h2j_engine *e, int n, const uint8_t *const *data, const size_t *sizes,
                                const h2j_out_opts2 *opts, uint8_t *out, size_t out_cap, size_t *out_off,
                                size_t *out_len, int *status);
int h2j_engine_transcode_opts2(h2j_engine *e, int n, const uint8_t *const *data, const size_t *sizes,
                               const h2j_out_opts2 *opts, uint8_t *out, size_t out_cap, size_t *out_off,
                               size_t *out_len, int *status);

/* Renditions: several JPEGs of one picture from one decode -- the full picture and its thumbnails.
 * Item i has nrend[i] renditions (1..H2J_MAX_RENDITIONS); opts, out_off, out_len and status are
 * item-major with sum(nrend) entries (frame errors: h2j_engine_frame_error with that index).  The item
 * is parsed and reconstructed once.  Rendition r of item i is byte for byte what the single-item call
 * with opts[r] returns.  A parse or decode failure fails every rendition of the item with the item's
 * status; invalid opts[r] fail that rendition alone with H2J_ERR_OUT_OPTS; -50 (output buffer too
 * small) is reported per rendition.  Renditions of one item that resolve to the same output are encoded
 * once and hold identical bytes.  A GPU chunk never separates the renditions of an item.  (DESIGN.md
 * "Renditions (K3p)": two or more of the scales 1/2, 1/4, 1/8 of one picture come from one read of it.) */
#define H2J_MAX_RENDITIONS 8
/* nrend[i] outside 1..H2J_MAX_RENDITIONS (or no nrend / opts): the call fails before anything runs */
#define H2J_ERR_RENDITIONS (-61)
int h2j_engine_transcode_multi(h2j_engine *e, int n, const uint8_t *const *data, const size_t *sizes,
                               const int32_t *nrend, const h2j_out_opts2 *opts, uint8_t *out, size_t out_cap,
                               size_t *out_off, size_t *out_len, int *status);
/* the asynchronous form: a ticket (> 0) for h2j_engine_wait, or H2J_ERR_RENDITIONS */
int64_t h2j_engine_submit_multi(h2j_engine *e, int n, const uint8_t *const *data, const size_t *sizes,
                                const int32_t *nrend, const h2j_out_opts2 *opts, uint8_t *out, size_t out_cap,
                                size_t *out_off, size_t *out_len, int *status);

/* Crop and cover: the JPEG of a window of the picture (DESIGN.md "Crop and cover").  A rendition may name
 * a window (crop_x, crop_y, crop_w, crop_h) in luma samples of the cropped W x H picture; its bytes are
 * exactly those the call with the same remaining options returns for a picture whose cropped planes are
 * the window's samples (luma rows y .. y+h-1, columns x .. x+w-1; chroma at half of each): scale_log2,
 * max_dim and fit act on w x h, K3s clamps at the window's last column and row, SOF0 carries the output
 * size.  crop_x, crop_y >= 0 and even; crop_w, crop_h >= 0 and even, 0: to the right / bottom edge
 * (w = W - x, h = H - y; all four 0: the whole picture); the resolved w, h >= 2, x + w <= W, y + h <= H.
 * Nothing is clamped: anything else fails that rendition alone with H2J_ERR_OUT_OPTS and a frame-error
 * message that names the picture's size.
 * H2J_FIT_COVER: the largest centred part of the window (the whole picture if none is named) with the
 * aspect of the box fit_w x fit_h (both >= 2), sized as H2J_FIT_STRETCH sizes it -- a square thumbnail of
 * a 16:9 picture.  Not with H2J_FIT_STRETCH, scale_log2 != 0 or max_dim != 0.  With box bw x bh, 64-bit
 * products and flooring divisions: if w bh >= h bw: ch = h, cw = clamp(2 (h bw / (2 bh)), 2, w); else
 * cw = w, ch = clamp(2 (w bh / (2 bw)), 2, h); x += 2 ((w - cw) / 4), y += 2 ((h - ch) / 4); the output
 * is h2j_fit_size(cw, ch, bw, bh, H2J_FIT_STRETCH).  1920 x 1080, cover 256 x 256: window (420, 0, 1080,
 * 1080), output 256 x 256.
 * A window that resolves to the whole picture is not a window: the job is the h2j_out_opts2 one. */
#define H2J_FIT_COVER 2
typedef struct {
    int32_t scale_log2, max_dim, fit_w, fit_h, flags; /* as h2j_out_opts2; flags may hold H2J_FIT_COVER */
    int32_t crop_x, crop_y, crop_w, crop_h;           /* window; all 0: the whole picture */
    int32_t reserved[3];                              /* must be 0 */
} h2j_out_opts3;                                      /* 48 bytes */

/* The window and size rule, a pure function (no engine, no GPU): for a cropped w x h picture (both even,
 * 2..65536) and options o, win[0..3] = the resolved window x, y, w, h (after cover) and *ow x *oh = the
 * output size (h2j_scaled_dim of the window at the resolved scale; h2j_fit_size of it; the cover size).
 * Returns 0, or H2J_ERR_OUT_OPTS for invalid options or a window outside the picture (nothing is written). */
int h2j_crop_window(int w, int h, const h2j_out_opts3 *o, int32_t *win, int *ow, int *oh);

/* h2j_engine_transcode_multi / h2j_engine_submit_multi with h2j_out_opts3; an h2j_out_opts2 item is the
 * h2j_out_opts3 item with the crop fields 0.  Renditions of one item that resolve to the same (window,
 * output) are encoded once; two or more of the scales 1/2, 1/4, 1/8 of the same window come from one read. */
int h2j_engine_transcode_multi3(h2j_engine *e, int n, const uint8_t *const *data, const size_t *sizes,
                                const int32_t *nrend, const h2j_out_opts3 *opts, uint8_t *out, size_t out_cap,
                                size_t *out_off, size_t *out_len, int *status);
int64_t h2j_engine_submit_multi3(h2j_engine *e, int n, const uint8_t *const *data, const size_t *sizes,
                                 const int32_t *nrend, const h2j_out_opts3 *opts, uint8_t *out, size_t out_cap,
                                 size_t *out_off, size_t *out_len, int *status);

/* Orientation: the JPEG of the picture rotated or mirrored on the GPU (DESIGN.md "Orientation (K3o)").
 * orient is 0..8: 0 and 1 mean "as decoded", 2..8 are the EXIF / TIFF orientation numbers, naming the
 * transform that makes the picture upright.  For a cropped plane P (H rows x W columns, numpy notation;
 * luma and both chroma planes alike) the oriented plane is
 *   2: P[:, ::-1] mirror left-right   3: P[::-1, ::-1] 180 degrees   4: P[::-1, :] mirror top-bottom
 *   5: P.T transpose   6: rot90(P, -1) 90 degrees clockwise   7: P[::-1, ::-1].T transverse
 *   8: rot90(P, 1) 90 degrees anticlockwise            (5..8: the oriented picture is H x W)
 * The oriented picture is the picture: the rendition's bytes are exactly those the same call with its
 * remaining options returns for a picture whose cropped planes are the oriented planes.  crop is in luma
 * samples of the oriented picture; cover, scale_log2, max_dim and fit act on it; SOF0 carries the
 * oriented output size.  The stage permutes samples in their own type: no new arithmetic.
 * H2J_ORIENT_AUTO: the orientation of the picture's display orientation SEI message (payload type 47,
 * H.264 D.2.27 / H.265 D.3.17: flip, then rotate anticlockwise), the last such message in front of picture
 * 0's first slice; 0 when there is none, when it is cancelled, malformed or truncated, or when its
 * rotation is no multiple of 90 degrees.  The SEI is never applied unasked: every call without orient
 * returns what it always returned.
 * orient outside -1..8 or non-zero reserved: that rendition fails alone with H2J_ERR_OUT_OPTS. */
#define H2J_ORIENT_AUTO (-1)
typedef struct {
    int32_t scale_log2, max_dim, fit_w, fit_h, flags; /* as h2j_out_opts3 */
    int32_t crop_x, crop_y, crop_w, crop_h;           /* window of the oriented picture */
    int32_t orient;                                   /* 0..8, or H2J_ORIENT_AUTO */
    int32_t reserved[6];                              /* must be 0 */
} h2j_out_opts4;                                      /* 64 bytes */
/* status of an oriented rendition when the kernel library in use has no orientation stage (an older
 * libh2j_hip.so selected beside this host library); the rendition fails alone */
#define H2J_ERR_NO_STAGE (-62)

/* The display orientation (0, 2..8) of picture 0 of an Annex-B stream of either codec, a pure function: it
 * reads NAL headers and SEI messages only (no entropy decode).  Negative for a stream that is neither codec. */
int h2j_stream_orientation(const uint8_t *data, size_t size);

/* h2j_crop_window for a decoded w x h picture with an orientation: win[0..3] and *ow x *oh are in the
 * coordinates of the oriented picture (h x w for orientations 5..8), *orient = the resolved orientation
 * (0 or 2..8; sei_orient, 0..8, is what H2J_ORIENT_AUTO resolves to).  The one place the rule lives.
 * Returns 0, or H2J_ERR_OUT_OPTS (nothing is written). */
int h2j_crop_window4(int w, int h, const h2j_out_opts4 *o, int sei_orient, int32_t *win, int *ow, int *oh, int *orient);

/* h2j_engine_transcode_multi3 / h2j_engine_submit_multi3 with h2j_out_opts4; an h2j_out_opts3 item is the
 * h2j_out_opts4 item with orient 0.  Renditions of one item that resolve to the same (orientation, window,
 * output) are encoded once; renditions with the same orientation share one pass of the orientation stage. */
int h2j_engine_transcode_multi4(h2j_engine *e, int n, const uint8_t *const *data, const size_t *sizes,
                                const int32_t *nrend, const h2j_out_opts4 *opts, uint8_t *out, size_t out_cap,
                                size_t *out_off, size_t *out_len, int *status);
int64_t h2j_engine_submit_multi4(h2j_engine *e, int n, const uint8_t *const *data, const size_t *sizes,
                                 const int32_t *nrend, const h2j_out_opts4 *opts, uint8_t *out, size_t out_cap,
                                 size_t *out_off, size_t *out_len, int *status);

/* Finishing: a fixed JPEG quantiser scale and an unsharp mask, per rendition (DESIGN.md "Finishing (K3u,
 * forced qscale)").  h2j_out_opts5 is h2j_out_opts4 with two of its reserved words named.
 * qscale: 0: the rate control's quantiser scale, as every other call.  2..31 (the range the rate control clips
 *   to): that scale -- the quantisation matrix and the quantiser (A.5) of it, the rate control
 *   formula skipped.  The scale equal to the one the rate control picks returns the bytes of the call without it.
 * sharpen: 0: off.  1..64: an unsharp mask of strength sharpen / 16 on the LUMA of the rendition's final 8-bit
 *   planes -- after orientation, window and scale / fit: the planes h2j_engine_decode_multi4 shows.  For the
 *   8-bit luma plane P (H x W, the JPEG size), coordinates clamped to the plane:
 *     S(x, y) = sum of w[dy][dx] P(x + dx, y + dy), dy, dx in -1..1, w = [1 2 1; 2 4 2; 1 2 1]
 *     D = 16 P - S          out = clip(P + ((sharpen D + 128) >> 8), 0, 255)       (arithmetic shift)
 *   integer arithmetic with one rounding, inside int32.  The chroma is the unsharpened 8-bit chroma.
 * The sharpened planes are the picture: the rendition's bytes are exactly those the same call without sharpen
 * returns for a picture whose 8-bit planes are the sharpened planes -- the rate control runs on the sharpened
 * luma when qscale is 0.  Every call without the two options returns the bytes it returned.
 * qscale outside {0, 2..31}, sharpen outside 0..64 or non-zero reserved: that rendition fails alone with
 * H2J_ERR_OUT_OPTS.  On a kernel library without the stage (h2j_gpu_finish, h2j_gpu_jpeg2) a rendition that names
 * either option fails alone with H2J_ERR_NO_STAGE. */
typedef struct {
    int32_t scale_log2, max_dim, fit_w, fit_h, flags; /* as h2j_out_opts4 */
    int32_t crop_x, crop_y, crop_w, crop_h;           /* window of the oriented picture */
    int32_t orient;                                   /* 0..8, or H2J_ORIENT_AUTO */
    int32_t qscale;                                   /* 0, or 2..31 */
    int32_t sharpen;                                  /* 0..64, in 1/16 */
    int32_t reserved[4];                              /* must be 0 */
} h2j_out_opts5;                                      /* 64 bytes */

/* h2j_crop_window4 with h2j_out_opts5: the same window, size and orientation, and the two range checks.
 * Returns 0, or H2J_ERR_OUT_OPTS (nothing is written). */
int h2j_crop_window5(int w, int h, const h2j_out_opts5 *o, int sei_orient, int32_t *win, int *ow, int *oh, int *orient);

/* h2j_engine_transcode_multi4 / h2j_engine_submit_multi4 with h2j_out_opts5; an h2j_out_opts4 item is the
 * h2j_out_opts5 item with qscale and sharpen 0 (the multi4 calls keep rejecting non-zero reserved words).
 * Renditions of one item that resolve to the same (orientation, window, output, qscale, sharpen) are encoded
 * once; renditions that differ only in qscale or sharpen each run the scale stage for themselves. */
int h2j_engine_transcode_multi5(h2j_engine *e, int n, const uint8_t *const *data, const size_t *sizes,
                                const int32_t *nrend, const h2j_out_opts5 *opts, uint8_t *out, size_t out_cap,
                                size_t *out_off, size_t *out_len, int *status);
int64_t h2j_engine_submit_multi5(h2j_engine *e, int n, const uint8_t *const *data, const size_t *sizes,
                                 const int32_t *nrend, const h2j_out_opts5 *opts, uint8_t *out, size_t out_cap,
                                 size_t *out_off, size_t *out_len, int *status);

/* RGB output: a rendition as raw pixels instead of a file (DESIGN.md "RGB output (K3c)").  h2j_out_opts6 is
 * h2j_out_opts5 with one more reserved word named.
 * format: H2J_FMT_JPEG (0): the JPEG, as every other call.  H2J_FMT_RGB8 / H2J_FMT_RGB8_PLANAR: the rendition's
 *   final 8-bit planes -- after orientation, window, scale / fit and sharpen: the planes
 *   h2j_engine_decode_multi5 shows and K4 would read -- converted to 8-bit RGB on the GPU.  For the planes Y (H x W)
 *   and Cb, Cr (H/2 x W/2), W and H even, the chroma upsampled with JFIF's centred siting by the 9-3-3-1 triangle
 *   filter at 16 x precision, all in int32 with one rounding:
 *     cx = x >> 1, nx = clamp(cx + ((x & 1) ? 1 : -1), 0, W/2 - 1);  cy, ny likewise with y, H/2
 *     C16(x, y) = 9 C[cy][cx] + 3 C[cy][nx] + 3 C[ny][cx] + C[ny][nx]
 *     db = Cb16 - 2048, dr = Cr16 - 2048
 *     R = clip(((Y << 20) + 91881 dr + (1 << 19)) >> 20, 0, 255)
 *     G = clip(((Y << 20) - 22554 db - 46802 dr + (1 << 19)) >> 20, 0, 255)
 *     B = clip(((Y << 20) + 116130 db + (1 << 19)) >> 20, 0, 255)                      (arithmetic shifts)
 *   The matrix is JFIF's (BT.601 full range) whatever the stream's VUI says: the RGB is what a viewer shows for the
 *   JPEG of the same rendition, without the JPEG loss.  No header.  H2J_FMT_RGB8: interleaved R, G, B, rows of
 *   exactly 3 W bytes (numpy (H, W, 3)); H2J_FMT_RGB8_PLANAR: an R plane, then G, then B, each W H bytes (numpy
 *   (3, H, W)).  3 W H bytes either way, at out + out_off[i], out_len[i] of them.
 * format outside 0..2, a raw format together with qscale (there is no quantiser) or non-zero reserved: that
 * rendition fails alone with H2J_ERR_OUT_OPTS.  On a kernel library without the stage (h2j_gpu_rgb) a raw
 * rendition fails alone with H2J_ERR_NO_STAGE.  A raw rendition that does not fit what is left of out_cap gets -50
 * like a JPEG; when its size alone decides that, the GPU stage does not run for it. */
#define H2J_FMT_JPEG 0
#define H2J_FMT_RGB8 1
#define H2J_FMT_RGB8_PLANAR 2
typedef struct {
    int32_t scale_log2, max_dim, fit_w, fit_h, flags; /* as h2j_out_opts5 */
    int32_t crop_x, crop_y, crop_w, crop_h;           /* window of the oriented picture */
    int32_t orient;                                   /* 0..8, or H2J_ORIENT_AUTO */
    int32_t qscale;                                   /* 0, or 2..31 (0 with a raw format) */
    int32_t sharpen;                                  /* 0..64, in 1/16 */
    int32_t format;                                   /* H2J_FMT_* */
    int32_t reserved[3];                              /* must be 0 */
} h2j_out_opts6;                                      /* 64 bytes */

/* h2j_crop_window5 with h2j_out_opts6: the same window, size and orientation, and the format checks.
 * Returns 0, or H2J_ERR_OUT_OPTS (nothing is written). */
int h2j_crop_window6(int w, int h, const h2j_out_opts6 *o, int sei_orient, int32_t *win, int *ow, int *oh, int *orient);

/* h2j_engine_transcode_multi5 / h2j_engine_submit_multi5 with h2j_out_opts6; an h2j_out_opts5 item is the
 * h2j_out_opts6 item with format 0 (the multi5 calls keep rejecting non-zero reserved words).  out_wh (may be NULL):
 * two entries per rendition, the output's W, H; written (else 0, 0) for every rendition of a parsed item whose
 * options resolve, JPEG renditions and those that got -50 too, so a caller can size a retry exactly.  A raw
 * rendition with the (orientation, window, output, sharpen) of a JPEG rendition of the same item reads that
 * rendition's planes: the scale stage runs once for both. */
int h2j_engine_transcode_multi6(h2j_engine *e, int n, const uint8_t *const *data, const size_t *sizes,
                                const int32_t *nrend, const h2j_out_opts6 *opts, uint8_t *out, size_t out_cap,
                                size_t *out_off, size_t *out_len, int *status, int32_t *out_wh);
int64_t h2j_engine_submit_multi6(h2j_engine *e, int n, const uint8_t *const *data, const size_t *sizes,
                                 const int32_t *nrend, const h2j_out_opts6 *opts, uint8_t *out, size_t out_cap,
                                 size_t *out_off, size_t *out_len, int *status, int32_t *out_wh);

/* Padded output: a rendition letterboxed to the exact size of its box (DESIGN.md "Padded output (K3b)").
 * h2j_out_opts7 is h2j_out_opts6 with two of its reserved words named.
 * pad: 0: off, as every other call.  1: the rendition is the box itself -- the picture part fitted inside it as the
 *   same options without pad fit it, centred, the rest filled with `background`.  Needs a two-sided box: fit_w >= 2
 *   and fit_h >= 2, with plain fit, H2J_FIT_STRETCH or H2J_FIT_COVER.
 * background: 0x00RRGGBB, the fill colour (8-bit sRGB as JFIF carries it); 0 is black.
 * The rule (all divisions floor): the picture part is the window, orientation and output ow x oh that
 * h2j_crop_window6 gives for the options without pad (always even, always inside the box).  The canvas is
 * BW = 2 (fit_w / 2), BH = 2 (fit_h / 2); the picture part sits at px = 2 ((BW - ow) / 4), py = 2 ((BH - oh) / 4)
 * (both even: the chroma sits at px / 2, py / 2 of a BW/2 x BH/2 plane).  The fill colour is JFIF's forward matrix in
 * 16.16, computed once on the host with arithmetic shifts (h2j_pad_colour):
 *     Y  = (19595 R + 38470 G +  7471 B + 32768) >> 16
 *     Cb = clip(((-11059 R - 21709 G + 32768 B + 32768) >> 16) + 128, 0, 255)
 *     Cr = clip((( 32768 R - 27439 G -  5329 B + 32768) >> 16) + 128, 0, 255)
 * so a grey (v, v, v) is (v, 128, 128), which the RGB formats turn back into (v, v, v) exactly.  The padded planes
 * are 8-bit planes Y (BH x BW) full of Y and Cb, Cr (BH/2 x BW/2) full of Cb, Cr, with the rendition's final 8-bit
 * planes -- after orientation, window, scale / fit and sharpen: the planes h2j_engine_decode_multi5 shows; the
 * unsharp mask never sees the border -- written over the rectangle at (px, py).
 * The padded planes are the picture: the rendition's bytes are exactly those the same call returns for a picture
 * whose 8-bit planes are the padded planes -- rate control, qscale and format included; SOF0 and out_wh carry BW x BH.
 * ow == BW and oh == BH: there is nothing to pad, and the rendition is the one without pad whatever background says.
 * Not built: upscaling to fill the box, a gravity other than the centre.
 * pad outside 0..1, background with bits above 23 set, background != 0 with pad 0, pad 1 without a two-sided box, a
 * canvas above H2J_PAD_MAX_SAMPLES (below) or non-zero reserved: that rendition fails alone with H2J_ERR_OUT_OPTS.  On a kernel library without the stage
 * (h2j_gpu_pad) a padded rendition fails alone with H2J_ERR_NO_STAGE.
 * The functions that take h2j_out_opts7 are declared in include/h2j_ext.h and exported by libH265ToJpegExt.so: this
 * header declares what libH265ToJpeg.so exports, and that list is fixed. */
/* The largest canvas, in luma samples: BW x BH <= H2J_PAD_MAX_SAMPLES (8192 x 8192, or as many samples in another
 * shape, e.g. 65534 x 1024).  Every other output is at most its decoded picture; a canvas is the caller's number, and it
 * is device memory (about 14.5 bytes a sample for a JPEG rendition).  The bound also keeps the canvas planes' byte
 * offsets -- at most 1.5 (BW + 15) BH < 2^27 -- far inside the int32 fields that carry them.  A padded rendition whose
 * box is larger fails alone with H2J_ERR_OUT_OPTS, whatever the picture's size. */
#define H2J_PAD_MAX_SAMPLES (1 << 26)
typedef struct {
    int32_t scale_log2, max_dim, fit_w, fit_h, flags; /* as h2j_out_opts6 */
    int32_t crop_x, crop_y, crop_w, crop_h;           /* window of the oriented picture */
    int32_t orient;                                   /* 0..8, or H2J_ORIENT_AUTO */
    int32_t qscale;                                   /* 0, or 2..31 (0 with a raw format) */
    int32_t sharpen;                                  /* 0..64, in 1/16 */
    int32_t format;                                   /* H2J_FMT_* */
    int32_t pad;                                      /* 0, or 1: letterbox to the box */
    int32_t background;                               /* 0x00RRGGBB (0 without pad) */
    int32_t reserved[1];                              /* must be 0 */
} h2j_out_opts7;                                      /* 64 bytes */

/* Colour: a rendition's planes normalised to JFIF's matrix and range (DESIGN.md "Colour (K3v)").
 * Without the option every JPEG and RGB array treats the decoded samples as JFIF -- BT.601, full range -- whatever
 * the stream says.  h2j_out_opts8 is h2j_out_opts7 with its last reserved word named.
 * colour: 0: off, as every other call.
 *   H2J_COLOUR_AUTO: the source's matrix and range are the stream's: the VUI video_signal_type of the H.264 / H.265
 *     SPS (video_full_range_flag; matrix_coefficients where colour_description_present_flag is set), or, in a HEIF
 *     file, the `nclx` colr property of the primary item, which wins over the VUI (a grid: the grid item's, else its
 *     tiles'; rICC / prof profiles are ignored).  matrix_coefficients 1 is BT.709; 5 and 6 are BT.601; 9 is BT.2020
 *     non-constant luminance; 2 (unspecified) or no signalling is BT.601 -- how the library reads such streams
 *     without the option, and swscale's default.  No range signalled is limited range (E.2.1 of both specs infers
 *     video_full_range_flag 0).  Any other matrix_coefficients (0 identity / GBR, 4, 7, 8 YCgCo, 10 constant
 *     luminance, 11 and above, reserved values) fails that rendition alone with H2J_ERR_OUT_OPTS, the value in its
 *     message: never a wrong picture.
 *   H2J_COLOUR_EXPLICIT | mc << 1 | full: the caller names the source, whatever the stream says: mc in {1, 5, 6, 9} as
 *     above, full 1 for full range, 0 for limited.
 * The rule.  (Kr, Kb) of the source matrix: BT.601 (0.299, 0.114), BT.709 (0.2126, 0.0722), BT.2020 (0.2627, 0.0593);
 * Kg = 1 - Kr - Kb; the target is Kr' = 0.299, Kb' = 0.114, Kg' = 0.587.  (oy, sy, sc) of the source range: limited
 * (16, 219, 224), full (0, 255, 255).  In exact rationals, rnd rounding to nearest with halves away from zero:
 *     a = 2 Kb'(1-Kb) - 2 Kg' Kb (1-Kb)/Kg        b = 2 Kr'(1-Kr) - 2 Kg' Kr (1-Kr)/Kg
 *     c = (2(1-Kb) - a) / (2(1-Kb'))              d = -b / (2(1-Kb'))
 *     e = -a / (2(1-Kr'))                         f = (2(1-Kr) - b) / (2(1-Kr'))
 *     g = 255 / sc
 *     LY = rnd(255/sy 2^20)   LB = rnd(a g 2^16)   LR = rnd(b g 2^16)
 *     CB = rnd(c g 2^16)      CR = rnd(d g 2^16)   RB = rnd(e g 2^16)   RR = rnd(f g 2^16)
 * (h2j_colour_coeffs of include/h2j_ext.h returns them).  The source is the rendition's 8-bit planes after orientation,
 * window and scale / fit -- the planes the unsharp mask would read; a source above 8 bits through K4's conversion
 * first.  With Cb16, Cr16 the 9-3-3-1 chroma of "RGB output" at luma position (x, y), 16 x precision, all shifts
 * arithmetic:
 *     Y'(x, y)  = clip((LY (Y - oy) + LB (Cb16 - 2048) + LR (Cr16 - 2048) + 2^19) >> 20, 0, 255)
 *     Cb'(i, j) = clip((CB (Cb - 128) + CR (Cr - 128) + (128 << 16) + 2^15) >> 16, 0, 255)
 *     Cr'(i, j) = clip((RB (Cb - 128) + RR (Cr - 128) + (128 << 16) + 2^15) >> 16, 0, 255)
 * BT.601 full range is exactly the identity: a rendition that resolves to it is the rendition without colour.
 * The normalised planes are the picture: the rendition's bytes are exactly those the same call without colour returns
 * for a picture whose 8-bit planes are the normalised planes -- the unsharp mask, the pad border (its colour is sRGB
 * and is not converted), rate control, qscale and format all act on them.
 * Not built: transfer functions and gamut (PQ / HLG tone mapping, BT.2020 -> sRGB primaries), ICC profiles, chroma
 * siting other than JFIF's centre, conversion at the source bit depth, colour tags in the JPEG.
 * Any other value of colour fails that rendition alone with H2J_ERR_OUT_OPTS.  On a kernel library without the stage
 * (h2j_gpu_colour) a converted rendition fails alone with H2J_ERR_NO_STAGE.
 * The functions that take h2j_out_opts8 are declared in include/h2j_ext.h and exported by libH265ToJpegExt.so. */
#define H2J_COLOUR_AUTO (-1)
#define H2J_COLOUR_EXPLICIT 0x100
typedef struct {
    int32_t scale_log2, max_dim, fit_w, fit_h, flags; /* as h2j_out_opts6 */
    int32_t crop_x, crop_y, crop_w, crop_h;           /* window of the oriented picture */
    int32_t orient;                                   /* 0..8, or H2J_ORIENT_AUTO */
    int32_t qscale;                                   /* 0, or 2..31 (0 with a raw format) */
    int32_t sharpen;                                  /* 0..64, in 1/16 */
    int32_t format;                                   /* H2J_FMT_* */
    int32_t pad;                                      /* 0, or 1: letterbox to the box */
    int32_t background;                               /* 0x00RRGGBB (0 without pad) */
    int32_t colour;                                   /* 0, H2J_COLOUR_AUTO, or H2J_COLOUR_EXPLICIT | mc << 1 | full */
} h2j_out_opts8;                                      /* 64 bytes */

/* Test / inspection entry points (one picture).
 * stage: 0 final decoded picture, 1 pre-loop-filter, 2 deblocked (pre-SAO).
 * planes_out: uint16 Y (w*h) then U, V ((w/2)*(h/2)) of the cropped picture.
 * info[0..2] = w, h, bit_depth. */
int h2j_engine_decode(h2j_engine *e, const uint8_t *data, size_t size, int stage, uint16_t *planes_out,
                      size_t cap_elems, int *info);
/* The same for picture `pick` of n pictures reconstructed as ONE GPU batch (the launch shapes of
 * a production chunk of n pictures: K1's picture pool with up to 4 pictures per workgroup at
 * n >= 1024), so parity tests can read planes from inside a bench-sized batch. */
int h2j_engine_decode_batch(h2j_engine *e, int n, const uint8_t *const *data, const size_t *sizes, int stage,
                            int pick, uint16_t *planes_out, size_t cap_elems, int *info);
/* JPEG coefficients int16 [mcu][6][64] zigzag of the decoded picture;
 * info[0..3] = w, h, qscale, nmcu. */
int h2j_engine_jpeg_coeffs(h2j_engine *e, const uint8_t *data, size_t size, int16_t *out, size_t cap_elems,
                           int *info);
/* Inspection of the scaled output: the 8-bit planes K4 reads for this picture -- Y (W_k * H_k)
 * then U, V ((W_k / 2) * (H_k / 2)), packed -- after K3s (at k = 0: the decoded planes through
 * the 8-bit conversion K4 applies).  info[0..3] = W_k, H_k, k (resolved), source bit depth. */
int h2j_engine_decode_scaled(h2j_engine *e, const uint8_t *data, size_t size, int scale_log2, int max_dim,
                             uint8_t *planes_out, size_t cap, int *info);
/* The same for exact-size output: the 8-bit planes K4 reads for this picture at the size
 * h2j_fit_size gives -- Y (W_o * H_o) then U, V ((W_o / 2) * (H_o / 2)), packed.
 * info[0..3] = W_o, H_o, mode (0 unscaled, 1..3 K3s at that scale_log2, 4 K3r), source bit depth. */
int h2j_engine_decode_resized(h2j_engine *e, const uint8_t *data, size_t size, int fit_w, int fit_h, int flags,
                              uint8_t *planes_out, size_t cap, int *info);
/* The same with all nrend renditions of the picture in flight, for rendition `pick`: the planes are what
 * the kernel that serves that rendition in such a batch wrote.  info as h2j_engine_decode_resized, and
 * mode 5: a K3s level written by K3p (the picture has two or more levels among its renditions). */
int h2j_engine_decode_multi(h2j_engine *e, const uint8_t *data, size_t size, int nrend, const h2j_out_opts2 *opts,
                            int pick, uint8_t *planes_out, size_t cap, int *info);
/* The same with h2j_out_opts3; info has 8 entries: [4..7] = the rendition's resolved window x, y, w, h.
 * Mode 5 then means: the window has two or more levels among the renditions (pyramids are per window). */
int h2j_engine_decode_multi3(h2j_engine *e, const uint8_t *data, size_t size, int nrend, const h2j_out_opts3 *opts,
                             int pick, uint8_t *planes_out, size_t cap, int *info);
/* The same with h2j_out_opts4; info has 10 entries: [0..7] as above with the window in the coordinates of the
 * oriented picture, [8] = the rendition's resolved orientation (0 or 2..8), [9] = the picture's SEI orientation.
 * At mode 0 the planes of an oriented rendition are the oriented planes K3o wrote, through K4's 8-bit conversion. */
int h2j_engine_decode_multi4(h2j_engine *e, const uint8_t *data, size_t size, int nrend, const h2j_out_opts4 *opts,
                             int pick, uint8_t *planes_out, size_t cap, int *info);
/* The same with h2j_out_opts5; info has 12 entries: [0..9] as above, [10] = the quantiser scale K4 used for the
 * rendition (the forced one, or the rate control's), [11] = its sharpen.  The planes are what K4 reads: those of a
 * sharpened rendition are the sharpened planes K3u wrote. */
int h2j_engine_decode_multi5(h2j_engine *e, const uint8_t *data, size_t size, int nrend, const h2j_out_opts5 *opts,
                             int pick, uint8_t *planes_out, size_t cap, int *info);
/* Timing of the batch the last h2j_engine_transcode / h2j_engine_wait returned, milliseconds:
 * [0] parse (host, wall, from submission)  [1] h2d  [2] recon  [3] deblock  [4] sao
 * [5] jpeg (GPU)  [6] d2h  [7] huffman (host, wall)  [8] total (wall)
 * [9] frames  [10] algorithmic bytes of the GPU pixel path  [11] GPU entropy
 * [12] K0 prep  [13] chunks  [14] record packing (host)  [15] parse (host, wall, first to last
 * picture of the batch: without the wait behind the previous batch)  [16..21] see STAT_KEYS in
 * h2j.py  [22] K3o / K3s / K3r / K3p / K3u orientation, scaled- and exact-size-output and finishing stage (GPU)  [23] renditions: JPEG outputs
 * of the batch ([9] frames stays the decoded pictures)  [24] parsed: pictures whose entropy decode ran
 * [25] raw bytes: the bytes of the raw (RGB) renditions delivered ([22] includes K3c, the RGB stage)
 * [26] pad bytes: the canvas bytes K3b wrote for the padded renditions -- per canvas its three 8-bit planes, rows of
 * whole 16-byte groups ([22] includes K3b, the padding stage)
 * [27] colour bytes: the plane bytes K3v wrote for the colour-converted renditions, counted the same way ([22] includes
 * K3v, the colour stage). */
int h2j_engine_stats(h2j_engine *e, double *out, int n);
/* Per chunk (one GPU launch of each stage) of the last h2j_engine_transcode, in order:
 * out[3i] pictures, out[3i+1] K1 ms, out[3i+2] K0..K5 ms (HIP events on the chunk's stream).
 * Returns the number of chunks (entries beyond max_chunks are not written). */
int h2j_engine_chunk_times(h2j_engine *e, double *out, int max_chunks);

/* In-memory and batch entry points beside IDecoder (the reference has only the
 * file-path call, /root/reference/export_inc/IDecoder.h:29).
 * Both go through the same process-wide batching engine as IDecoder, so
 * concurrent callers share GPU batches.
 * h2j_h265_to_jpeg_mem: one Annex-B still (H.264 or H.265) -> JPEG bytes in
 *   *jpeg (malloc'ed, release with h2j_free), 0 on success, < 0 on failure.
 * h2j_h265_to_jpeg_batch: n (input, output) file pairs transcoded as one
 *   batch; ok[i] = 1 where output i was written (may be NULL); returns the
 *   number written.  Per-file behaviour (empty paths, unreadable input, LOG
 *   lines) is that of IDecoder::H265ToJpeg. */
int h2j_h265_to_jpeg_mem(const uint8_t *data, size_t size, uint8_t **jpeg, size_t *jpeg_len);
int h2j_h265_to_jpeg_batch(const char *const *in_paths, const char *const *out_paths, int n, int *ok);
/* h2j_h265_to_jpeg_mem with scaled output (h2j_out_opts above): concurrent callers with
 * different scales still share GPU batches. */
int h2j_h265_to_jpeg_mem_scaled(const uint8_t *data, size_t size, int scale_log2, int max_dim, uint8_t **jpeg,
                                size_t *jpeg_len);
/* h2j_h265_to_jpeg_mem with exact-size output (h2j_out_opts2 above: fit_w, fit_h, flags);
 * concurrent callers with different sizes still share GPU batches. */
int h2j_h265_to_jpeg_mem_fit(const uint8_t *data, size_t size, int fit_w, int fit_h, int flags, uint8_t **jpeg,
                             size_t *jpeg_len);
/* h2j_h265_to_jpeg_mem with nrend renditions of the picture (h2j_engine_transcode_multi: one decode).  It
 * goes through the process-wide batching engine, so concurrent callers still share GPU batches.
 * jpeg[r] is malloc'ed (release with h2j_free), or NULL where status[r] < 0.  Returns 0 if the call
 * ran (per-rendition results in status), H2J_ERR_RENDITIONS for nrend outside 1..H2J_MAX_RENDITIONS. */
int h2j_h265_to_jpeg_mem_multi(const uint8_t *data, size_t size, int nrend, const h2j_out_opts2 *opts, uint8_t **jpeg,
                               size_t *jpeg_len, int *status);
/* the same with h2j_out_opts3 (crop and cover): concurrent callers with different windows still share GPU batches */
int h2j_h265_to_jpeg_mem_multi3(const uint8_t *data, size_t size, int nrend, const h2j_out_opts3 *opts, uint8_t **jpeg,
                                size_t *jpeg_len, int *status);
/* the same with h2j_out_opts4 (orientation): concurrent callers with different orientations still share GPU batches */
int h2j_h265_to_jpeg_mem_multi4(const uint8_t *data, size_t size, int nrend, const h2j_out_opts4 *opts, uint8_t **jpeg,
                                size_t *jpeg_len, int *status);
/* the same with h2j_out_opts5 (finishing): concurrent callers with different finishing options still share GPU batches */
int h2j_h265_to_jpeg_mem_multi5(const uint8_t *data, size_t size, int nrend, const h2j_out_opts5 *opts, uint8_t **jpeg,
                                size_t *jpeg_len, int *status);
/* the same with h2j_out_opts6 (RGB output): jpeg[r] of a raw rendition holds its jpeg_len[r] = 3 W H pixel bytes;
 * out_wh (may be NULL) as in h2j_engine_transcode_multi6 */
int h2j_h265_to_jpeg_mem_multi6(const uint8_t *data, size_t size, int nrend, const h2j_out_opts6 *opts, uint8_t **jpeg,
                                size_t *jpeg_len, int *status, int32_t *out_wh);
void h2j_free(void *p);

/* Library self-description (version, arch, build). */
const char *h2j_version(void);

#ifdef __cplusplus
}
#endif
#endif
