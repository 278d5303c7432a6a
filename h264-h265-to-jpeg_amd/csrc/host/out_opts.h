// Output options (include/h2j.h): the one rule set that says what a rendition's options mean -- the public option
// types widened to h2j_out_opts7, their validity, and the output (window, scale or size, orientation, finishing,
// format, padding) they resolve to on a picture of a given size.  Pure arithmetic on include/*.h and FrameJob::Output: no
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

// h2j_out_opts7 is the type the rules below are written on: h2j_out_opts6 with two of its reserved words named (pad,
// background).  An item of an older type is its to_opts6 form with those two 0 and every word that is reserved there
// folded into the one reserved word left, so a non-zero one stays a non-zero reserved word
extern const h2j_out_opts7 kPlainOutput7;
h2j_out_opts7 widen7(const h2j_out_opts6& o);
inline const h2j_out_opts7& to_opts7(const h2j_out_opts7& o) { return o; }
template <typename T>
h2j_out_opts7 to_opts7(const T& o) { return widen7(to_opts6(o)); }
template <typename T>
std::vector<h2j_out_opts7> to_opts7(int n, const T* o) {  // o null: all plain
    std::vector<h2j_out_opts7> v(static_cast<size_t>(std::max(n, 0)), kPlainOutput7);
    for (int i = 0; o && i < n; i++) v[i] = to_opts7(o[i]);
    return v;
}

bool reserved_zero(const h2j_out_opts6& o);
bool reserved_zero(const h2j_out_opts7& o);
bool fit_valid(int fit_w, int fit_h, int flags);
bool finish_valid(const h2j_out_opts7& o);
bool format_valid(const h2j_out_opts7& o);
bool pad_valid(const h2j_out_opts7& o);
// what can be said of the options before the picture's size is known; the window's place in the picture is
// checked by resolve_output
bool out_opts_valid(const h2j_out_opts7& o);

int resolve_scale(const h2j_out_opts7& o, int w, int h);
// the orientation (0, 2..8) the options name for a picture whose display orientation SEI says sei_orient
int resolve_orient(const h2j_out_opts7& o, int sei_orient);
// the output of a W x H picture (its parsed, cropped size) with options that passed out_opts_valid
FrameJob::Output resolve_output(const h2j_out_opts7& o, int W, int H, int sei_orient);
// W, H: the parsed picture's cropped size (0: not parsed)
std::string out_opts_message(const h2j_out_opts7& o, int W = 0, int H = 0, int sei_orient = 0);

// h2j_fit_size, and h2j_crop_window .. h2j_crop_window6 on an item of any option type
int fit_size(int w, int h, int fit_w, int fit_h, int flags, int* ow, int* oh);
int crop_window6(int w, int h, const h2j_out_opts6* o, int sei_orient, int32_t* win, int* ow, int* oh, int* orient);
// h2j_crop_window7: *ow x *oh is the canvas of a padded output, place = px, py and the picture part's w, h
int crop_window7(int w, int h, const h2j_out_opts7* o, int sei_orient, int32_t* win, int* ow, int* oh, int* orient, int32_t* place);
// h2j_pad_colour: the fill bytes Y, Cb, Cr of a background 0x00RRGGBB
int pad_colour(uint32_t rgb, int* ycc);
template <typename T>
int crop_window(int w, int h, const T* o, int sei_orient, int32_t* win, int* ow, int* oh, int* orient) {
    if (!o) return H2J_ERR_OUT_OPTS;
    const h2j_out_opts6 o6 = to_opts6(*o);
    return crop_window6(w, h, &o6, sei_orient, win, ow, oh, orient);
}

}  // namespace h2j
