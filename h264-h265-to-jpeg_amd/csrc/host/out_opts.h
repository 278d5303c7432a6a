// Output options (include/h2j.h): the one rule set that says what a rendition's options mean -- the public option
// types widened to h2j_out_opts8, their validity, and the output (window, scale or size, orientation, finishing,
// format, padding, colour) they resolve to on a picture of a given size.  Pure arithmetic on include/*.h and FrameJob::Output: no
// thread, no GPU call, no engine.  Whether the kernel library has the stage an output needs is the engine's matter.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "h2j.h"
#include "job.h"

namespace h2j {

extern const h2j_out_opts6 kPlainOutput;  // the JPEG at the decoded size

// h2j_out_opts6 is the one option type behind the C ABI.  Each older type is the item whose later fields are 0; a word
// that was reserved in the older type and became a field since must still be 0 there: a non-zero one stays a
// non-zero reserved word
h2j_out_opts6 to_opts6(const h2j_out_opts& o);
h2j_out_opts6 to_opts6(const h2j_out_opts2& o);
h2j_out_opts6 to_opts6(const h2j_out_opts3& o);
h2j_out_opts6 to_opts6(const h2j_out_opts4& o);
h2j_out_opts6 to_opts6(const h2j_out_opts5& o);
inline const h2j_out_opts6& to_opts6(const h2j_out_opts6& o) { return o; }
template <typename T>
std::vector<h2j_out_opts6> to_opts6(int n, const T* o) {  // o null: all plain
    std::vector<h2j_out_opts6> v(static_cast<size_t>(std::max(n, 0)), kPlainOutput);
    for (int i = 0; o && i < n; i++) v[i] = to_opts6(o[i]);
    return v;
}

// h2j_out_opts8 is the type the rules below are written on: h2j_out_opts6 with its three reserved words named (pad,
// background, colour).  An item of an older type is its to_opts6 form with those 0 -- and, where a word that is reserved
// there is non-zero, the colour kColourReserved, which is what a non-zero reserved word looks like here: such an item
// stays invalid, and is told so in the words it always was
constexpr int32_t kColourReserved = INT32_MIN;
extern const h2j_out_opts8 kPlainOutput8;
h2j_out_opts8 widen8(const h2j_out_opts6& o);
h2j_out_opts8 widen8(const h2j_out_opts7& o);
inline const h2j_out_opts8& to_opts8(const h2j_out_opts8& o) { return o; }
inline h2j_out_opts8 to_opts8(const h2j_out_opts7& o) { return widen8(o); }
template <typename T>
h2j_out_opts8 to_opts8(const T& o) { return widen8(to_opts6(o)); }
template <typename T>
std::vector<h2j_out_opts8> to_opts8(int n, const T* o) {  // o null: all plain
    std::vector<h2j_out_opts8> v(static_cast<size_t>(std::max(n, 0)), kPlainOutput8);
    for (int i = 0; o && i < n; i++) v[i] = to_opts8(o[i]);
    return v;
}

bool reserved_zero(const h2j_out_opts6& o);
bool reserved_zero(const h2j_out_opts8& o);
bool fit_valid(int fit_w, int fit_h, int flags);
bool finish_valid(const h2j_out_opts8& o);
bool format_valid(const h2j_out_opts8& o);
bool pad_valid(const h2j_out_opts8& o);
bool colour_valid(const h2j_out_opts8& o);
// what can be said of the options before the picture's size is known; the window's place in the picture is
// checked by resolve_output
bool out_opts_valid(const h2j_out_opts8& o);

int resolve_scale(const h2j_out_opts8& o, int w, int h);
// the orientation (0, 2..8) the options name for a picture whose display orientation SEI says sei_orient
int resolve_orient(const h2j_out_opts8& o, int sei_orient);
// the output of a W x H picture (its parsed, cropped size) with options that passed out_opts_valid
// (stream_colour: what the stream signals -- primaries, transfer, matrix_coefficients, full range, as FrameJob::colour;
// null: nothing, 2 / 2 / 2 / 0 -- for H2J_COLOUR_AUTO)
FrameJob::Output resolve_output(const h2j_out_opts8& o, int W, int H, int sei_orient, const int* stream_colour = nullptr);
// W, H: the parsed picture's cropped size (0: not parsed)
std::string out_opts_message(const h2j_out_opts8& o, int W = 0, int H = 0, int sei_orient = 0, const int* stream_colour = nullptr);

// Colour (include/h2j.h "Colour").  The source the option names for a stream that signals stream_colour: *matrix 1, 6 or
// 9 (5 is 6) and *full 1 / 0.  Returns 0, or H2J_ERR_OUT_OPTS: an invalid word, or a matrix_coefficients value the
// library does not convert (*matrix is then that value).  colour 0 gives 6 / 1: JFIF, nothing to convert
int resolve_colour(const h2j_out_opts8& o, const int* stream_colour, int* matrix, int* full);
// h2j_colour_coeffs: oy, LY, LB, LR, CB, CR, RB, RR of a source matrix (1, 5, 6, 9) and range, in exact integers
int colour_coeffs(int matrix, int full, int32_t* k);

// h2j_fit_size, and h2j_crop_window .. h2j_crop_window6 on an item of any option type
int fit_size(int w, int h, int fit_w, int fit_h, int flags, int* ow, int* oh);
int crop_window6(int w, int h, const h2j_out_opts6* o, int sei_orient, int32_t* win, int* ow, int* oh, int* orient);
// h2j_crop_window7: *ow x *oh is the canvas of a padded output, place = px, py and the picture part's w, h
int crop_window7(int w, int h, const h2j_out_opts7* o, int sei_orient, int32_t* win, int* ow, int* oh, int* orient, int32_t* place);
int crop_window8(int w, int h, const h2j_out_opts8* o, int sei_orient, int32_t* win, int* ow, int* oh, int* orient, int32_t* place);
// h2j_pad_colour: the fill bytes Y, Cb, Cr of a background 0x00RRGGBB
int pad_colour(uint32_t rgb, int* ycc);
template <typename T>
int crop_window(int w, int h, const T* o, int sei_orient, int32_t* win, int* ow, int* oh, int* orient) {
    if (!o) return H2J_ERR_OUT_OPTS;
    const h2j_out_opts6 o6 = to_opts6(*o);
    return crop_window6(w, h, &o6, sei_orient, win, ow, oh, orient);
}

}  // namespace h2j
