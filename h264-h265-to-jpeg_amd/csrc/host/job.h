// Host-side container for one picture's job records (see include/h2j_jobs.h).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "h2j.h"
#include "h2j_gpu.h"
#include "h2j_jobs.h"

namespace h2j {

struct FrameJob {
    h2j_frame hdr{};
    std::vector<h2j_tu> tus;
    std::vector<h2j_coef> coefs;
    std::vector<h2j_ctb> ctbs;
    std::vector<h2j_slice> slices;
    std::vector<uint8_t> sl;  // scaling factors (2032 B) when hdr.scaling_list
    int error = 0;            // 0 ok, <0 parse error
    std::string message;
    int threads = 1;          // threads the parser may use inside this picture (independent slices)
    // the SPS signals output reordering (H.264 VUI max_num_reorder_frames > 0, H.265
    // sps_max_num_reorder_pics[HighestTid] > 0): FFmpeg holds the picture back until more
    // pictures or a flush arrive (only H2J_STRICT_REFERENCE acts on it)
    bool reorder_delay = false;
    // H.264 PAFF: picture 0 is a field pair (two field pictures).  FFmpeg outputs the frame after
    // the second field; the reference sends one packet (one field) and returns false (only
    // H2J_STRICT_REFERENCE acts on it)
    bool field_pair = false;
    // the display orientation SEI in front of the picture's first slice as an orientation 0, 2..8
    // (include/h2j.h "Orientation"; 0: none, cancelled or unusable).  Only H2J_ORIENT_AUTO acts on it
    int sei_orient = 0;
    // what the stream signals of its colour: colour_primaries, transfer_characteristics, matrix_coefficients and the
    // full-range flag of the SPS's VUI video_signal_type, or the nclx colr property of a HEIF file, which wins (2, 2, 2,
    // 0 where nothing is signalled).  Only H2J_COLOUR_AUTO acts on the last two; the first two are reported
    int colour[4] = {2, 2, 2, 0};
    // the item's outputs, one per rendition it asks for (a plain item: one), resolved by the engine after
    // the parse from the rendition's options and the parsed size (resolve_output), or that rendition's own
    // error (invalid options fail it alone).  A job that did not parse has none
    struct Output {
        // the JPEG at 1/2^scale_log2 of the decoded size; exact-size output: H2J_SCALE_RESAMPLE and the
        // JPEG is fit_w x fit_h (a size K3s makes is given to it as scale_log2 1..3)
        int scale_log2 = 0, fit_w = 0, fit_h = 0, error = 0;
        // the window of the cropped picture the output shows (crop and cover), in luma samples; the scale
        // and the fit act on it.  windowed is false for the whole picture, whatever named it: such an
        // output is the one without a window
        int win_x = 0, win_y = 0, win_w = 0, win_h = 0;
        bool windowed = false;
        // the orientation of the picture the window lies in: 0 as decoded, 2..8 (include/h2j.h); the window
        // is then in the coordinates of the oriented picture.  0: the job is the one without an orientation
        int orient = 0;
        // finishing (include/h2j.h "Finishing"): the quantiser scale K4 is to use (0: the rate control's) and the
        // strength of the unsharp mask K3u applies to the output's 8-bit luma (0: none)
        int qscale = 0, sharpen = 0;
        // RGB output (include/h2j.h "RGB output"): 0 the JPEG; H2J_FMT_RGB8 / H2J_FMT_RGB8_PLANAR: the output's final
        // 8-bit planes as RGB pixels, made by K3c
        int format = 0;
        // padded output (include/h2j.h "Padded output"): pad 1: K3b writes the output's final 8-bit planes into a
        // canvas of box_w x box_h at (pad_x, pad_y), the rest the fill bytes (Y, Cb, Cr); an output with nothing to pad
        // has pad 0: it is the one without the option
        int pad = 0, box_w = 0, box_h = 0, pad_x = 0, pad_y = 0;
        uint8_t fill[3] = {0, 0, 0};
        // colour (include/h2j.h "Colour"): 0: the planes as decoded; else H2J_COLOUR_EXPLICIT | matrix << 1 | full, the
        // resolved source K3v normalises to JFIF's -- an output whose source is BT.601 full range has 0: it is the one
        // without the option.  col_matrix (1, 6, 9; 0 without the option) and col_full: what the option resolved to
        int colour = 0, col_matrix = 0, col_full = 0;
        int32_t col_k[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // with colour != 0: K3v's constants (h2j_colour.k)
        // the luma size of the output's picture part (all of it without pad; the scale stage sizes from it): the
        // window's at the resolved scale, or the fit size
        int out_w() const { return scale_log2 == H2J_SCALE_RESAMPLE ? fit_w : h2j_scaled_dim(win_w, scale_log2); }
        int out_h() const { return scale_log2 == H2J_SCALE_RESAMPLE ? fit_h : h2j_scaled_dim(win_h, scale_log2); }
        // the luma size of what the caller gets (SOF0, out_wh, raw sizes): the canvas of a padded output
        int canvas_w() const { return pad ? box_w : out_w(); }
        int canvas_h() const { return pad ? box_h : out_h(); }
    };
    Output outs[H2J_MAX_RENDITIONS];
    int nouts = 0;
    int out_base = 0;  // index of the item's first rendition in the batch's output arrays
    // a HEIF input's items rewritten as Annex-B streams (heif.h), owned here so the parse can outlive the
    // demuxer; untouched by clear(), which the parsers call on the job they fill, and released by the next
    // parse_any on this job (HEIF or not), so a reused slot never keeps a large file's bytes
    std::vector<uint8_t> demuxed;

    void clear() {
        hdr = h2j_frame{};
        tus.clear();
        coefs.clear();
        ctbs.clear();
        slices.clear();
        sl.clear();
        error = 0;
        message.clear();
        reorder_delay = false;
        field_pair = false;
        sei_orient = 0;
        colour[0] = colour[1] = colour[2] = 2;
        colour[3] = 0;
        nouts = 0;
    }
};

// Offsets of the scaling-factor tables inside FrameJob::sl
enum { H2J_SL_S0 = 0, H2J_SL_S1 = 48, H2J_SL_S2 = 240, H2J_SL_S3 = 1008, H2J_SL_BYTES = 2032 };
// H.264 weight-scale tables inside FrameJob::sl (raster order): 4x4 intra Y/Cb/Cr, 8x8 intra Y
enum { H2J_SL264_4 = 0, H2J_SL264_8 = 48, H2J_SL264_BYTES = 112 };

// Parse the first picture of an HEVC Annex-B stream into job records.
// Returns 0 on success.
int hevc_parse_picture(const uint8_t* data, size_t size, FrameJob& job);
// Same for H.264.
int h264_parse_picture(const uint8_t* data, size_t size, FrameJob& job);
// A HEIF grid (rows x cols tile pictures as Annex-B streams, raster order; output out_w x out_h) parsed into the
// job records of one tiled canvas picture.  Tiles parse side by side when job.threads > 1; the records are the same.
int hevc_parse_grid(const uint8_t* const* tiles, const size_t* sizes, int rows, int cols, int out_w, int out_h, FrameJob& job);
// A HEIF file (heif.h: is_heif): its primary item demuxed into job.demuxed and parsed by the calls above; irot /
// imir become job.sei_orient.  heif_orientation: that orientation alone (0, 2..8; negative: the demuxer's status)
int heif_parse_picture(const uint8_t* data, size_t size, FrameJob& job);
int heif_orientation(const uint8_t* data, size_t size);
// What a stream signals of its colour without decoding it (FrameJob::colour): the first SPS that parses of an Annex-B
// stream (false: none does); a HEIF file's nclx colr property, else its item's SPS (a negative status: the demuxer's, or
// -100 for an item without an SPS)
bool hevc_stream_colour(const uint8_t* data, size_t size, int* colour);
bool h264_stream_colour(const uint8_t* data, size_t size, int* colour);
int heif_stream_colour(const uint8_t* data, size_t size, int* colour);

}  // namespace h2j
