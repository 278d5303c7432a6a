/*
 * h2j_gpu.h — thin C ABI of libh2j_hip.so, the MI355X (gfx950) pixel
 * pipeline.  Plain pointers and sizes; no torch / HIP types in signatures
 * (streams and events are opaque void*).
 *
 * Boundary: these entry points replace what the reference does inside
 * FFmpeg after entropy decoding, i.e. the arithmetic behind
 *   avcodec_send_packet/avcodec_receive_frame (/root/reference/src/Decoder.cpp:324,342):
 *     dequant + inverse transform + intra prediction   -> h2j_gpu_recon
 *     deblocking                                       -> h2j_gpu_deblock
 *     SAO                                              -> h2j_gpu_sao
 *   avcodec_send_frame (/root/reference/src/Encoder.cpp:250), mjpeg encoder:
 *     pad + MB variance + rate control + FDCT + quantiser + zigzag + symbol
 *     statistics                                       -> h2j_gpu_jpeg
 * The host (libH265ToJpeg.so) builds the optimal Huffman tables from the
 * statistics and emits the JPEG bitstream (avcodec_receive_packet, :259).
 *
 * All functions return 0 on success, a negative code on failure; the text
 * of the last failure is available from h2j_gpu_last_error().
 */
#ifndef H2J_GPU_H
#define H2J_GPU_H
#include <stddef.h>
#include <stdint.h>

#include "h2j_jobs.h"

#ifdef __cplusplus
extern "C" {
#endif

/* device / memory / stream plumbing */
int h2j_gpu_device_count(void);
int h2j_gpu_set_device(int device);
/* PCI bus id "dddd:bb:dd.f" of a device (locates its NUMA node in sysfs for host-thread pinning) */
int h2j_gpu_pci_bus_id(int device, char *buf, int len);
void *h2j_gpu_malloc(size_t bytes);
int h2j_gpu_free(void *p);
int h2j_gpu_mem_info(size_t *free_bytes, size_t *total_bytes); /* current device */
void *h2j_gpu_host_alloc(size_t bytes); /* pinned */
int h2j_gpu_host_free(void *p);
void *h2j_gpu_stream_create(void);
int h2j_gpu_stream_destroy(void *stream);
int h2j_gpu_stream_sync(void *stream);
int h2j_gpu_memcpy_h2d(void *dst, const void *src, size_t bytes, void *stream);
int h2j_gpu_memcpy_d2h(void *dst, const void *src, size_t bytes, void *stream);
int h2j_gpu_memset(void *dst, int value, size_t bytes, void *stream);
void *h2j_gpu_event_create(void);
int h2j_gpu_event_destroy(void *ev);
int h2j_gpu_event_record(void *ev, void *stream);
/* `stream` runs nothing enqueued after this call until `ev` (recorded on another stream) has completed */
int h2j_gpu_stream_wait_event(void *stream, void *ev);
float h2j_gpu_event_elapsed_ms(void *start, void *stop);
const char *h2j_gpu_last_error(void);

#ifdef __cplusplus
/* HEVC residual planes (K0 writes, K1 reads) in quadrant tiles: each component in tiles of
 * 2^q x 2^q int16 samples (q = the K1 quadrant size: min(log2ctb, 5) for luma, one less for
 * chroma), tiles in raster order, planes Y, Cb, Cr back to back.  A K1 quadrant is then one
 * contiguous tile (2 KB luma, 512 B per chroma plane) and every TB lies inside one tile.
 * (constexpr: host and device code share it) */
constexpr int h2j_res_q(int log2ctb, int c) { return (log2ctb < 5 ? log2ctb : 5) - (c ? 1 : 0); }
constexpr long long h2j_res_tiles(int n, int q) { return (n + (1 << q) - 1) >> q; }
constexpr long long h2j_res_plane(int w, int h, int q) { return (h2j_res_tiles(w, q) * h2j_res_tiles(h, q)) << (2 * q); }
/* int16 elements of the three tiled planes of a w x h 4:2:0 picture */
constexpr long long h2j_res_elems(int w, int h, int log2ctb) {
    return h2j_res_plane(w, h, h2j_res_q(log2ctb, 0)) + 2 * h2j_res_plane(w / 2, h / 2, h2j_res_q(log2ctb, 1));
}
/* K3 SAO sums the JPEG rate control's MB variances of a picture (K4a skips it) when the picture
 * has SAO (its own output plane) and its 16x16 output MB grid is aligned with the CTB grid.
 * (constexpr: host and device code share it) */
constexpr bool h2j_sao_folds_variance(const h2j_frame &f) {
    return f.codec == H2J_CODEC_HEVC && f.pic2 != f.pic && (f.crop_x & 15) == 0 && (f.crop_y & 15) == 0 &&
           (f.out_w & 15) == 0;
}
/* Scaled output (DESIGN.md "Scaled output"): luma size of an n-sample dimension at scale k, 2 * ceil(n / 2^(k+1)):
 * always even, so the JPEG's 4:2:0 chroma is exactly half of it; k = 0 gives n (n even). */
constexpr int h2j_scaled_dim(int n, int k) { return k ? 2 * ((n + (2 << k) - 1) >> (k + 1)) : n; }
/* bytes per row of a scaled plane of w samples: whole 16-byte groups (K3s stores dwords, K4c loads 8 bytes) */
constexpr int h2j_spic_stride(int w) { return (w + 15) & ~15; }
/* K3s workgroups (256 lanes: 64 dwords of 4 output samples x 4 rows) of one plane and of a picture */
constexpr int h2j_k3s_plane_tiles(int w, int h) { return ((((w + 3) >> 2) + 63) >> 6) * ((h + 3) >> 2); }
constexpr int h2j_k3s_tiles(int jpeg_w, int jpeg_h) {
    return h2j_k3s_plane_tiles(jpeg_w, jpeg_h) + 2 * h2j_k3s_plane_tiles(jpeg_w / 2, jpeg_h / 2);
}
/* K3r workgroups (256 lanes: 4 waves, each 64 dwords of 4 output samples x a strip of 8 output rows) */
constexpr int h2j_k3r_plane_tiles(int w, int h) { return ((((w + 3) >> 2) + 63) >> 6) * ((h + 31) >> 5); }
constexpr int h2j_k3r_tiles(int jpeg_w, int jpeg_h) {
    return h2j_k3r_plane_tiles(jpeg_w, jpeg_h) + 2 * h2j_k3r_plane_tiles(jpeg_w / 2, jpeg_h / 2);
}
/* K3o (orientation): elements per row of an oriented plane of w samples of pel bytes: whole 64-byte groups */
constexpr int h2j_opic_stride(int w, int pel) { return ((w * pel + 63) & ~63) / pel; }
/* K3o workgroups (256 lanes) of one oriented ow x oh plane: mirrors move 256 16-byte row segments each,
 * transposes one 64 x 64 tile each; and of a picture (three planes) */
constexpr int h2j_k3o_plane_tiles(int ow, int oh, int pel, bool transposing) {
    return transposing ? ((ow + 63) >> 6) * ((oh + 63) >> 6) : (((ow * pel + 15) >> 4) * oh + 255) >> 8;
}
constexpr int h2j_k3o_tiles(int ow, int oh, int pel, bool transposing) {
    return h2j_k3o_plane_tiles(ow, oh, pel, transposing) + 2 * h2j_k3o_plane_tiles(ow / 2, oh / 2, pel, transposing);
}
/* K3u (finishing) workgroups (256 lanes: 64 dwords of 4 output samples x 4 lane rows of H2J_K3U_ROWS output
 * rows each) of one plane and of a picture */
#define H2J_K3U_ROWS 4
constexpr int h2j_k3u_plane_tiles(int w, int h) { return ((((w + 3) >> 2) + 63) >> 6) * ((h + 4 * H2J_K3U_ROWS - 1) / (4 * H2J_K3U_ROWS)); }
constexpr int h2j_k3u_tiles(int jpeg_w, int jpeg_h) {
    return h2j_k3u_plane_tiles(jpeg_w, jpeg_h) + 2 * h2j_k3u_plane_tiles(jpeg_w / 2, jpeg_h / 2);
}
/* K3c (RGB output) workgroups (256 lanes: 64 lanes of 4 adjacent pixels x 4 lane rows; lane row j makes the output
 * rows 2 j - 1 and 2 j, which share the chroma rows j - 1 and j: h / 2 + 1 lane rows) of one w x h output */
constexpr int h2j_k3c_tiles(int w, int h) { return ((((w + 3) >> 2) + 63) >> 6) * (((h >> 1) + 1 + 3) >> 2); }
/* K3b (padded output) workgroups (256 lanes: 64 dwords of 4 canvas samples x 4 lane rows of H2J_K3B_ROWS canvas rows
 * each) of one canvas plane of w samples a row -- its rows' whole 16-byte groups are written -- and of a bw x bh canvas */
#define H2J_K3B_ROWS 4
constexpr int h2j_k3b_plane_tiles(int w, int h) { return (((h2j_spic_stride(w) >> 2) + 63) >> 6) * ((h + 4 * H2J_K3B_ROWS - 1) / (4 * H2J_K3B_ROWS)); }
constexpr int h2j_k3b_tiles(int bw, int bh) { return h2j_k3b_plane_tiles(bw, bh) + 2 * h2j_k3b_plane_tiles(bw / 2, bh / 2); }
/* K3v (colour) workgroups (256 lanes) of one w x h output.  The matrix class: 64 lanes of 8 adjacent luma samples x 4
 * lane rows; lane row j makes the luma rows 2 j - 1 and 2 j from the chroma rows j - 1 and j, and converts chroma row
 * j: h / 2 + 1 lane rows.  The range-only class: per plane, 64 dwords of 4 samples x 4 lane rows of H2J_K3V_ROWS rows */
#define H2J_K3V_ROWS 4
constexpr int h2j_k3v_matrix_tiles(int w, int h) { return ((((w + 7) >> 3) + 63) >> 6) * (((h >> 1) + 1 + 3) >> 2); }
constexpr int h2j_k3v_plane_tiles(int w, int h) { return ((((w + 3) >> 2) + 63) >> 6) * ((h + 4 * H2J_K3V_ROWS - 1) / (4 * H2J_K3V_ROWS)); }
constexpr int h2j_k3v_range_tiles(int w, int h) { return h2j_k3v_plane_tiles(w, h) + 2 * h2j_k3v_plane_tiles(w / 2, h / 2); }
/* K3p's grid is K3s's over the coarsest level of the picture's pyramid (h2j_k3s_tiles of that level's
 * size): a lane makes 4 adjacent outputs of that level and the finer levels' outputs under them */
#endif

/* JPEG symbol stream (production path): per frame, one tile of H2J_JTILE_BYTES per 256 blocks
 * at h2j_frame.jcoef (the dense int16 plane occupies the same region on the inspection path). */
#define H2J_JSYM_MAX 68
#define H2J_JTILE_BYTES (H2J_JSYM_MAX * 256 * 4 + 256 + 512)

#define H2J_SAO_GROUPS 4
/* K3s launches: sample type (8-bit, high bit depth) x scale (1/2, 1/4, 1/8); then K3r's (exact-size
 * output): 8-bit, high bit depth */
#define H2J_SCALE_CLASSES 8
#define H2J_K3R_CLASS0 6
/* K3p launches: sample type (8-bit, high bit depth) x coarsest level (2, 3) */
#define H2J_PYR_CLASSES 4

/* One batch of pictures resident in HBM.  All pointers are device pointers. */
typedef struct {
    int32_t nframes;
    int32_t max_w, max_h;       /* max coded luma size over the batch */
    int32_t max_mcu;            /* max JPEG MCUs over the batch */
    int32_t max_ntu;            /* max transform-block records over the batch */
    int32_t has_hevc, has_h264; /* codecs present in the batch */
    int32_t max_ctbs;           /* max CTBs of one HEVC picture over the batch */
    int32_t k1wgs;              /* H.264 K1 workgroups (sum of h2j_frame.k1bands over H.264 pictures) */
    const uint32_t *k1map;      /* H.264 K1 workgroup -> (frame << 8) | band, dependency order */
    int32_t hevc_pels;          /* HEVC sample types present: bit 0 8-bit, bit 1 high bit depth */
    int32_t k1all_n;            /* entries of k1all */
    const uint32_t *k1all;      /* mixed-batch K1 workgroups, longest chains first: HEVC pictures
                                   (1u << 31) | (frame << 8), then H.264 (frame << 8) | band */
    const h2j_frame *frames;
    const h2j_tu *tus;
    const h2j_coef *coefs;
    const h2j_ctb *ctbs;
    const h2j_slice *slices;
    const uint8_t *sl;
    uint8_t *arena;             /* pictures, maps, JPEG coefficients + stats */
    /* JPEG entropy stage (h2j_gpu_entropy) */
    uint8_t *seg;               /* entropy-coded segment pool, frames packed at jstat.seg_off */
    uint64_t seg_cap;           /* pool bytes */
    uint32_t *tile_bits;        /* scratch: nframes x ceil(max_mcu*6/256) */
    uint64_t *seg_total;        /* device scalar: pool bytes used (16-byte units x16) */
    int32_t jpeg_dense;         /* 1: K4 writes the dense int16 coefficient plane (inspection), no K5 */
    int32_t k4a_frames;         /* frames whose MB variances K4a sums (the others are summed by K3 SAO,
                                   h2j_sao_folds_variance); 0: K4a is not launched */
    int32_t has_mbaff;          /* H.264 MBAFF frames present (K1 runs h2j_k1_recon_h264_mbaff for them) */
    int32_t h264_pels;          /* non-MBAFF H.264 sample types present: bit 0 8-bit, bit 1 high bit depth */
    /* K3 SAO: one launch per CTB-count class of the HEVC pictures with SAO (a mixed batch's 720p,
       1080p and 4K pictures each get a grid of their own width instead of the largest one's) */
    int32_t sao_groups;         /* launches (0..H2J_SAO_GROUPS) */
    int32_t sao_first[H2J_SAO_GROUPS], sao_count[H2J_SAO_GROUPS], sao_ctbs[H2J_SAO_GROUPS];
    const uint32_t *sao_map;    /* frame indices of the HEVC pictures with SAO, most CTBs first */
    /* H.264 K1 launch of kAvcK1Waves-wave workgroups (h2j_k1_recon_h264): tall pictures in bands of
       as many rows as the workgroup has waves (one row round per band), band-major */
    int32_t k1wgs8;
    const uint32_t *k1map8;     /* workgroup -> (frame << 8) | band of 8 macroblock rows */
    /* the HEVC entries of k1all alone, same order: a mixed batch's HEVC K1 (h2j_k1_recon_any) beside
       the H.264 K1 (h2j_k1_recon_h264 on k1map8) on a companion stream */
    int32_t k1hevc_n;
    const uint32_t *k1hevc;
    /* JPEG source views of the frames: what K4 (variance, FDCT) and K5 read as "the picture".  An
       unscaled frame is its own view; a scaled frame's view is the 8-bit scaled picture K3s wrote
       at h2j_scaled.spic (crop 0, out_w x out_h = jpeg_w x jpeg_h, the spic strides and plane offsets, bit
       depth 8, pic == pic2 so that K4a sums its variances), so the K4 / K5 kernels run the same
       code for both kinds.  The engine builds them (ChunkPlan::view, chunk_plan.cpp); == frames, or NULL,
       when no picture of the batch is scaled.  A picture with several renditions has one view per
       distinct output (each with its own jcoef and jstat, the first the frame's own); the engine then
       runs K4 / K5 on a second descriptor whose nframes counts the views and whose frames are the views */
    const h2j_frame *jframes;
    /* K3s: the scaled pictures (h2j_scaled), grouped by class (3 * (sample type: 0 8-bit, 1 high
       bit depth) + scale_log2 - 1), one launch per class present; scale_tiles: the most workgroups
       one picture of the class needs (h2j_k3s_tiles).  K3 SAO may have summed such a picture's
       unscaled MB variances (h2j_sao_folds_variance knows nothing of scaling); K3s clears the sum and
       K4a, which sees pic == pic2 in the view, sums those of the scaled picture.
       K3r: the exact-size pictures (scale_log2 == H2J_SCALE_RESAMPLE) are the classes H2J_K3R_CLASS0 +
       sample type of the same map, their scale_tiles from h2j_k3r_tiles; the rest holds for them alike */
    const h2j_scaled *scale_map;
    int32_t scale_first[H2J_SCALE_CLASSES], scale_count[H2J_SCALE_CLASSES], scale_tiles[H2J_SCALE_CLASSES];
    /* K3p: the pictures with two or more K3s levels among their renditions (h2j_pyramid; their levels are
       not in scale_map), grouped by class (2 * sample type + coarsest level - 2), one launch per class
       present; pyr_tiles: the most workgroups one picture of the class needs (h2j_k3s_tiles of its coarsest
       level).  NULL: none */
    const h2j_pyramid *pyr_map;
    int32_t pyr_first[H2J_PYR_CLASSES], pyr_count[H2J_PYR_CLASSES], pyr_tiles[H2J_PYR_CLASSES];
} h2j_gpu_batch;

/* K0 + K1: K0 (all TUs in parallel) availability masks, CTB->TU ranges,
 * deblocking maps, PCM samples and residuals (dequantisation + inverse
 * transform) into frame.res; K1 (CTB-row wavefront, one workgroup per
 * picture) intra prediction + residual -> the pre-loop-filter picture in
 * frame.pic.  HEVC and H.264. */
int h2j_gpu_recon(const h2j_gpu_batch *b, void *stream);
/* the two halves of h2j_gpu_recon: K0 alone, then K1 alone */
int h2j_gpu_prep(const h2j_gpu_batch *b, void *stream);
int h2j_gpu_predict(const h2j_gpu_batch *b, void *stream);
/* Diagnostics: K1 cycle counters of a -DH2J_PROF build (`make prof`); -1 otherwise. */
int h2j_gpu_prof(unsigned long long *out, int n, int reset);
/* K2: deblocking (vertical edges, then horizontal edges), in place on frame.pic */
int h2j_gpu_deblock(const h2j_gpu_batch *b, void *stream);
/* K3: SAO frame.pic -> frame.pic2 (copies when SAO is off) */
int h2j_gpu_sao(const h2j_gpu_batch *b, void *stream);
/* K3s: box-filter downscale of the scaled pictures (b->scale_map), cropped frame.pic2 ->
 * the 8-bit planes at h2j_scaled.spic, K3r: area-average resampling of the exact-size
 * pictures of the same map, and K3p: every K3s level of the pictures of b->pyr_map from one read;
 * no launch when the batch has none */
int h2j_gpu_scale(const h2j_gpu_batch *b, void *stream);
/* K3o: the oriented sources (h2j_orient, a device array), grouped by class (2 * (sample type: 0 8-bit, 1 high
 * bit depth) + (transposing: orientations 5..8)): cropped frame.pic2 -> the planes at h2j_orient.opic, rotated
 * or mirrored, in the frame's sample type.  first / count / tiles: per class (host arrays of
 * H2J_ORIENT_CLASSES), tiles the most workgroups one picture of the class needs (h2j_k3o_tiles); one launch
 * per class present.  Runs after K3 SAO and before h2j_gpu_scale, whose kernels read the oriented planes
 * through frame copies.  A kernel library older than the stage lacks the symbol: the host library resolves it
 * when it loads and fails oriented renditions alone (H2J_ERR_NO_STAGE) */
#define H2J_ORIENT_CLASSES 4
int h2j_gpu_orient(const h2j_gpu_batch *b, const h2j_orient *map, const int32_t *first, const int32_t *count,
                   const int32_t *tiles, void *stream);
/* K3u: the sharpened outputs (h2j_finish, a device array), grouped by source class (0: the 8-bit planes K3s /
 * K3r / K3p wrote, h2j_finish.wide; 1: another 8-bit source; 2: a 16-bit source): source planes -> the 8-bit
 * planes at h2j_finish.dst, the luma through the 3 x 3 unsharp mask (DESIGN.md "Finishing (K3u, forced
 * qscale)"), the chroma copied through K4's 8-bit conversion.  first / count / tiles: per class (host arrays of
 * H2J_FINISH_CLASSES), tiles the most workgroups one output of the class needs (h2j_k3u_tiles); one launch per
 * class present.  Runs after h2j_gpu_scale, whose outputs it reads, and before K4.  A kernel library older
 * than the stage lacks the symbol (and h2j_gpu_jpeg2): the host library resolves both when it loads and fails
 * finishing renditions alone (H2J_ERR_NO_STAGE) */
#define H2J_FINISH_CLASSES 3
int h2j_gpu_finish(const h2j_gpu_batch *b, const h2j_finish *map, const int32_t *first, const int32_t *count,
                   const int32_t *tiles, void *stream);
/* K3c: the raw (RGB) outputs (h2j_rgb, a device array), grouped by source class as K3u's (0: the 8-bit planes K3s /
 * K3r / K3p / K3u wrote, h2j_rgb.wide; 1: another 8-bit source; 2: a 16-bit source): source planes -> w x h 8-bit
 * RGB pixels at h2j_rgb.dst_base + dst_off, interleaved or planar, tightly packed (DESIGN.md "RGB output (K3c)":
 * JFIF's matrix, the chroma through the 9-3-3-1 triangle filter).  first / count / tiles: per class (host arrays
 * of H2J_RGB_CLASSES), tiles the most workgroups one output of the class needs (h2j_k3c_tiles); one launch per
 * class present.  Runs after h2j_gpu_finish, whose outputs it may read, and before K4; out of place.  A kernel
 * library older than the stage lacks the symbol: the host library resolves it when it loads and fails raw
 * renditions alone (H2J_ERR_NO_STAGE) */
#define H2J_RGB_CLASSES 3
int h2j_gpu_rgb(const h2j_gpu_batch *b, const h2j_rgb *map, const int32_t *first, const int32_t *count,
                const int32_t *tiles, void *stream);
/* K3b: the padded outputs (h2j_pad, a device array), grouped by source class as K3u's (0: the 8-bit planes K3s / K3r /
 * K3p / K3u wrote, h2j_pad.wide; 1: another 8-bit source; 2: a 16-bit source): the fill bytes and the source planes ->
 * the canvas planes at h2j_pad.dst (DESIGN.md "Padded output (K3b)").  first / count / tiles: per class (host arrays
 * of H2J_PAD_CLASSES), tiles the most workgroups one canvas of the class needs (h2j_k3b_tiles); one launch per class
 * present.  Runs after h2j_gpu_finish, whose outputs it may read, and before h2j_gpu_rgb and K4, which may read the
 * canvas; out of place.  A kernel library older than the stage lacks the symbol: the host library resolves it when it
 * loads and fails padded renditions alone (H2J_ERR_NO_STAGE) */
#define H2J_PAD_CLASSES 3
int h2j_gpu_pad(const h2j_gpu_batch *b, const h2j_pad *map, const int32_t *first, const int32_t *count,
                const int32_t *tiles, void *stream);
/* K3v: the colour-converted outputs (h2j_colour, a device array), grouped by class = 2 x source class (as K3u's: 0: the
 * 8-bit planes K3s / K3r / K3p wrote, h2j_colour.wide; 1: another 8-bit source; 2: a 16-bit source) + h2j_colour.matrix:
 * the source planes -> planes in JFIF's matrix and range at h2j_colour.dst (DESIGN.md "Colour (K3v)").  first / count /
 * tiles: per class (host arrays of H2J_COLOUR_CLASSES), tiles the most workgroups one output of the class needs
 * (h2j_k3v_range_tiles, h2j_k3v_matrix_tiles); one launch per class present.  Runs after h2j_gpu_scale, whose outputs
 * it may read, and before h2j_gpu_finish, h2j_gpu_pad, h2j_gpu_rgb and K4, which may read its; out of place.  A kernel
 * library older than the stage lacks the symbol: the host library resolves it when it loads and fails colour-converted
 * renditions alone (H2J_ERR_NO_STAGE) */
#define H2J_COLOUR_CLASSES 6
int h2j_gpu_colour(const h2j_gpu_batch *b, const h2j_colour *map, const int32_t *first, const int32_t *count,
                   const int32_t *tiles, void *stream);
/* K4: JPEG forward path on the frames' JPEG source views (frame.pic2, or h2j_scaled.spic of a scaled
 * picture) -> frame.jcoef / frame.jstat
 * (variance, rate control, FDCT + quantiser + zigzag, symbol histograms) */
int h2j_gpu_jpeg(const h2j_gpu_batch *b, void *stream);
/* h2j_gpu_jpeg with the quantiser scale of some views set by the caller: qforce is a device array of one int32
 * per view of b (b->nframes entries), 0: the rate control's scale, 2..31: that scale -- K4b skips the rate
 * control formula for the view and jstat.qscale holds the value (jstat.lambda: 118 x it).  NULL: h2j_gpu_jpeg */
int h2j_gpu_jpeg2(const h2j_gpu_batch *b, const int32_t *qforce, void *stream);
/* K4d alone: Huffman symbol histograms of frame.jcoef -> jstat.hist */
int h2j_gpu_histogram(const h2j_gpu_batch *b, void *stream);
/* K5: optimal Huffman tables (jstat.bits/val/code/len) and the entropy-coded
 * payload of every frame, packed into b->seg at jstat.seg_off (jstat.nbytes
 * bytes, 1-padded, no 0xFF stuffing).  *b->seg_total = bytes used. */
int h2j_gpu_entropy(const h2j_gpu_batch *b, void *stream);

#ifdef __cplusplus
}
#endif
#endif
