// The calls behind libH265ToJpegExt.so (api_ext.cpp).  libH265ToJpeg.so's exported C names are a fixed list
// (tests/golden/abi/exports.txt): the entry points added since (include/h2j_ext.h: padded output's, colour's) are exported by
// a second, thin library beside it, which forwards to these functions of the host library.
#pragma once
#include <cstddef>
#include <cstdint>

#include "h2j_ext.h"

namespace h2j {

// h2j_engine_submit_multi7 (latency false) and h2j_engine_transcode_multi7 (latency true: submit and wait)
int64_t submit_multi7(h2j_engine* e, int n, const uint8_t* const* data, const size_t* sizes, const int32_t* nrend, const h2j_out_opts7* opts,
                      uint8_t* out, size_t out_cap, size_t* out_off, size_t* out_len, int* status, int32_t* out_wh, bool latency);
// h2j_engine_decode_multi7
int decode_multi7(h2j_engine* e, const uint8_t* data, size_t size, int nrend, const h2j_out_opts7* opts, int pick, uint8_t* planes_out,
                  size_t cap, int* info);
// h2j_h265_to_jpeg_mem_multi7
int mem_multi7(const uint8_t* data, size_t size, int nrend, const h2j_out_opts7* opts, uint8_t** jpeg, size_t* jpeg_len, int* status,
               int32_t* out_wh);
// the same with h2j_out_opts8 (colour): h2j_engine_submit_multi8 / _transcode_multi8, h2j_engine_decode_multi8,
// h2j_h265_to_jpeg_mem_multi8
int64_t submit_multi8(h2j_engine* e, int n, const uint8_t* const* data, const size_t* sizes, const int32_t* nrend, const h2j_out_opts8* opts,
                      uint8_t* out, size_t out_cap, size_t* out_off, size_t* out_len, int* status, int32_t* out_wh, bool latency);
int decode_multi8(h2j_engine* e, const uint8_t* data, size_t size, int nrend, const h2j_out_opts8* opts, int pick, uint8_t* planes_out,
                  size_t cap, int* info);
int mem_multi8(const uint8_t* data, size_t size, int nrend, const h2j_out_opts8* opts, uint8_t** jpeg, size_t* jpeg_len, int* status,
               int32_t* out_wh);
// h2j_stream_colour
int stream_colour(const uint8_t* data, size_t size, int32_t* info);
// (h2j_crop_window7, h2j_pad_colour and h2j_colour_coeffs forward to out_opts.h: crop_window7, pad_colour, colour_coeffs)

}  // namespace h2j
