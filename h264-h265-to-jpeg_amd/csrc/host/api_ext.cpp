// libH265ToJpegExt.so: the C entry points of include/h2j_ext.h, younger than libH265ToJpeg.so's fixed export list
// (api_ext.h) -- padded output's and colour's.  Each forwards to the host library, which this library links; nothing else lives here.
#include "api_ext.h"
#include "out_opts.h"

extern "C" {

int h2j_engine_transcode_multi7(h2j_engine* e, int n, const uint8_t* const* data, const size_t* sizes, const int32_t* nrend, const h2j_out_opts7* opts,
                                uint8_t* out, size_t out_cap, size_t* out_off, size_t* out_len, int* status, int32_t* out_wh) {
    return static_cast<int>(h2j::submit_multi7(e, n, data, sizes, nrend, opts, out, out_cap, out_off, out_len, status, out_wh, true));
}
int64_t h2j_engine_submit_multi7(h2j_engine* e, int n, const uint8_t* const* data, const size_t* sizes, const int32_t* nrend, const h2j_out_opts7* opts,
                                 uint8_t* out, size_t out_cap, size_t* out_off, size_t* out_len, int* status, int32_t* out_wh) {
    return h2j::submit_multi7(e, n, data, sizes, nrend, opts, out, out_cap, out_off, out_len, status, out_wh, false);
}
int h2j_engine_decode_multi7(h2j_engine* e, const uint8_t* data, size_t size, int nrend, const h2j_out_opts7* opts, int pick,
                             uint8_t* planes_out, size_t cap, int* info) {
    return h2j::decode_multi7(e, data, size, nrend, opts, pick, planes_out, cap, info);
}
int h2j_h265_to_jpeg_mem_multi7(const uint8_t* data, size_t size, int nrend, const h2j_out_opts7* opts, uint8_t** jpeg, size_t* jpeg_len,
                                int* status, int32_t* out_wh) {
    return h2j::mem_multi7(data, size, nrend, opts, jpeg, jpeg_len, status, out_wh);
}
int h2j_crop_window7(int w, int h, const h2j_out_opts7* o, int sei_orient, int32_t* win, int* ow, int* oh, int* orient, int32_t* place) {
    return h2j::crop_window7(w, h, o, sei_orient, win, ow, oh, orient, place);
}
int h2j_pad_colour(uint32_t rgb, int* ycc) { return h2j::pad_colour(rgb, ycc); }

int h2j_engine_transcode_multi8(h2j_engine* e, int n, const uint8_t* const* data, const size_t* sizes, const int32_t* nrend, const h2j_out_opts8* opts,
                                uint8_t* out, size_t out_cap, size_t* out_off, size_t* out_len, int* status, int32_t* out_wh) {
    return static_cast<int>(h2j::submit_multi8(e, n, data, sizes, nrend, opts, out, out_cap, out_off, out_len, status, out_wh, true));
}
int64_t h2j_engine_submit_multi8(h2j_engine* e, int n, const uint8_t* const* data, const size_t* sizes, const int32_t* nrend, const h2j_out_opts8* opts,
                                 uint8_t* out, size_t out_cap, size_t* out_off, size_t* out_len, int* status, int32_t* out_wh) {
    return h2j::submit_multi8(e, n, data, sizes, nrend, opts, out, out_cap, out_off, out_len, status, out_wh, false);
}
int h2j_engine_decode_multi8(h2j_engine* e, const uint8_t* data, size_t size, int nrend, const h2j_out_opts8* opts, int pick,
                             uint8_t* planes_out, size_t cap, int* info) {
    return h2j::decode_multi8(e, data, size, nrend, opts, pick, planes_out, cap, info);
}
int h2j_h265_to_jpeg_mem_multi8(const uint8_t* data, size_t size, int nrend, const h2j_out_opts8* opts, uint8_t** jpeg, size_t* jpeg_len,
                                int* status, int32_t* out_wh) {
    return h2j::mem_multi8(data, size, nrend, opts, jpeg, jpeg_len, status, out_wh);
}
int h2j_stream_colour(const uint8_t* data, size_t size, int32_t* info) { return h2j::stream_colour(data, size, info); }
int h2j_colour_coeffs(int matrix, int full, int32_t* k) { return h2j::colour_coeffs(matrix, full, k); }

}  // extern "C"
