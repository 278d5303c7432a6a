/*
 * h2j_ext.h -- C ABI of libH265ToJpegExt.so: the entry points younger than libH265ToJpeg.so's fixed export list.
 *
 * include/h2j.h declares what libH265ToJpeg.so exports, and that list of names does not change.  Entry points added
 * since are exported by libH265ToJpegExt.so, a thin library built beside it that forwards to it: link
 * -lH265ToJpegExt -lH265ToJpeg, or open both from an FFI binding (h2j.py does).  The types and constants they use are
 * in include/h2j.h.  So far: padded output (h2j.h "Padded output", h2j_out_opts7; DESIGN.md "Padded output (K3b)") and
 * colour (h2j.h "Colour", h2j_out_opts8; DESIGN.md "Colour (K3v)").
 */
#ifndef H2J_EXT_H
#define H2J_EXT_H
#include "h2j.h"

#ifdef __cplusplus
extern "C" {
#endif

/* h2j_crop_window6 with h2j_out_opts7: win and *orient as there; *ow x *oh is the output's size -- the canvas of a
 * padded rendition -- and place[0..3] = px, py and the picture part's w, h inside it (0, 0, *ow, *oh when nothing is
 * padded).  Returns 0, or H2J_ERR_OUT_OPTS (nothing is written). */
int h2j_crop_window7(int w, int h, const h2j_out_opts7 *o, int sei_orient, int32_t *win, int *ow, int *oh, int *orient,
                     int32_t place[4]);
/* The fill colour of a background 0x00RRGGBB as the three plane bytes ycc[0..2] = Y, Cb, Cr (the formulas of h2j.h "Padded output").
 * Returns 0, or H2J_ERR_OUT_OPTS for bits above 23 or no ycc (nothing is written). */
int h2j_pad_colour(uint32_t rgb, int ycc[3]);

/* h2j_engine_transcode_multi6 / h2j_engine_submit_multi6 with h2j_out_opts7; an h2j_out_opts6 item is the
 * h2j_out_opts7 item with pad and background 0 (the multi6 calls keep rejecting non-zero reserved words).  A padded
 * rendition reads the planes of its picture part where any other rendition of the item -- padded or not -- has the
 * same (orientation, window, output, sharpen): the scale stage and the unsharp mask run once.  Padded renditions
 * of one picture part with one box and one colour share one canvas, a JPEG and a raw one alike. */
int h2j_engine_transcode_multi7(h2j_engine *e, int n, const uint8_t *const *data, const size_t *sizes,
                                const int32_t *nrend, const h2j_out_opts7 *opts, uint8_t *out, size_t out_cap,
                                size_t *out_off, size_t *out_len, int *status, int32_t *out_wh);
int64_t h2j_engine_submit_multi7(h2j_engine *e, int n, const uint8_t *const *data, const size_t *sizes,
                                 const int32_t *nrend, const h2j_out_opts7 *opts, uint8_t *out, size_t out_cap,
                                 size_t *out_off, size_t *out_len, int *status, int32_t *out_wh);

/* h2j_engine_decode_multi5 with h2j_out_opts7; info has 18 entries: [0..11] as there with [0], [1] the output's size (the canvas of
 * a padded rendition) and [2] the mode of its picture part, [12] = 1 if the rendition was padded (0: pad off, or nothing
 * to pad), [13..16] = px, py and the picture part's w, h, [17] = the fill colour as Y | Cb << 8 | Cr << 16.  The planes
 * are what K4 reads: those of a padded rendition are the padded planes K3b wrote. */
int h2j_engine_decode_multi7(h2j_engine *e, const uint8_t *data, size_t size, int nrend, const h2j_out_opts7 *opts,
                             int pick, uint8_t *planes_out, size_t cap, int *info);

/* h2j_h265_to_jpeg_mem_multi6 with h2j_out_opts7 (padded output): out_wh holds the canvas of a padded rendition */
int h2j_h265_to_jpeg_mem_multi7(const uint8_t *data, size_t size, int nrend, const h2j_out_opts7 *opts, uint8_t **jpeg,
                                size_t *jpeg_len, int *status, int32_t *out_wh);

/* Colour (h2j.h "Colour").  The multi7 calls with h2j_out_opts8; an h2j_out_opts7 item is the h2j_out_opts8 item with
 * colour 0 (the multi7 calls keep rejecting a non-zero reserved word).  Renditions of one (orientation, window, output)
 * and one resolved (matrix, range) share one conversion, a JPEG and a raw one alike; a converted rendition reads the
 * scale stage's planes of an unconverted rendition of the same geometry. */
int h2j_engine_transcode_multi8(h2j_engine *e, int n, const uint8_t *const *data, const size_t *sizes,
                                const int32_t *nrend, const h2j_out_opts8 *opts, uint8_t *out, size_t out_cap,
                                size_t *out_off, size_t *out_len, int *status, int32_t *out_wh);
int64_t h2j_engine_submit_multi8(h2j_engine *e, int n, const uint8_t *const *data, const size_t *sizes,
                                 const int32_t *nrend, const h2j_out_opts8 *opts, uint8_t *out, size_t out_cap,
                                 size_t *out_off, size_t *out_len, int *status, int32_t *out_wh);
/* h2j_engine_decode_multi7 with h2j_out_opts8; info has 21 entries: [0..17] as there, [18] the resolved source matrix
 * (matrix_coefficients: 1, 6 or 9; 0 with colour off), [19] the resolved range (1 full, 0 limited), [20] = 1 if the
 * rendition was converted (0: colour off, or BT.601 full range -- nothing to convert).  The planes are what K4 reads. */
int h2j_engine_decode_multi8(h2j_engine *e, const uint8_t *data, size_t size, int nrend, const h2j_out_opts8 *opts,
                             int pick, uint8_t *planes_out, size_t cap, int *info);
int h2j_h265_to_jpeg_mem_multi8(const uint8_t *data, size_t size, int nrend, const h2j_out_opts8 *opts, uint8_t **jpeg,
                                size_t *jpeg_len, int *status, int32_t *out_wh);
/* What a stream signals, without decoding it (pure: no engine): info[0..3] = colour_primaries, transfer_characteristics,
 * matrix_coefficients, full range (1 / 0), from the first SPS's VUI of an Annex-B stream or, in a HEIF file, the nclx
 * colr property (which wins over the VUI); 2 / 2 / 2 / 0 where nothing is signalled.  Returns 0, or a negative status:
 * -1 for a null argument, -100 for bytes that are no stream, the demuxer's for a HEIF file it refuses. */
int h2j_stream_colour(const uint8_t *data, size_t size, int32_t info[4]);
/* The constants of a source matrix (matrix_coefficients 1, 5, 6 or 9) and range (full 1 / 0): k[0..7] = oy, LY, LB, LR,
 * CB, CR, RB, RR of h2j.h "Colour", computed with integers.  Returns 0, or H2J_ERR_OUT_OPTS (nothing is written). */
int h2j_colour_coeffs(int matrix, int full, int32_t k[8]);

#ifdef __cplusplus
}
#endif
#endif
