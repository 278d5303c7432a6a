#include "out_opts.h"

#include <utility>

namespace h2j {

const h2j_out_opts6 kPlainOutput = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, {0, 0, 0}};

h2j_out_opts6 to_opts6(const h2j_out_opts& o) { return h2j_out_opts6{o.scale_log2, o.max_dim, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, {0, 0, 0}}; }
h2j_out_opts6 to_opts6(const h2j_out_opts2& o) {
    return h2j_out_opts6{o.scale_log2, o.max_dim, o.fit_w, o.fit_h, o.flags, 0, 0, 0, 0, 0, 0, 0, 0, {o.reserved[0], o.reserved[1], o.reserved[2]}};
}
h2j_out_opts6 to_opts6(const h2j_out_opts3& o) {
    return h2j_out_opts6{o.scale_log2, o.max_dim, o.fit_w, o.fit_h, o.flags, o.crop_x, o.crop_y, o.crop_w, o.crop_h, 0, 0, 0, 0,
                         {o.reserved[0], o.reserved[1], o.reserved[2]}};
}
// (qscale, sharpen and format took over reserved[0..2] of h2j_out_opts4, format reserved[0] of h2j_out_opts5)
h2j_out_opts6 to_opts6(const h2j_out_opts4& o) {
    return h2j_out_opts6{o.scale_log2, o.max_dim, o.fit_w, o.fit_h, o.flags, o.crop_x, o.crop_y, o.crop_w, o.crop_h, o.orient, 0, 0, 0,
                         {o.reserved[0] | o.reserved[1] | o.reserved[2] | o.reserved[3], o.reserved[4], o.reserved[5]}};
}
h2j_out_opts6 to_opts6(const h2j_out_opts5& o) {
    return h2j_out_opts6{o.scale_log2, o.max_dim, o.fit_w, o.fit_h, o.flags, o.crop_x, o.crop_y, o.crop_w, o.crop_h, o.orient,
                         o.qscale, o.sharpen, 0, {o.reserved[0] | o.reserved[1], o.reserved[2], o.reserved[3]}};
}

const h2j_out_opts8 kPlainOutput8 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
// (pad, background and colour took over reserved[0..2] of h2j_out_opts6, colour reserved[0] of h2j_out_opts7)
h2j_out_opts8 widen8(const h2j_out_opts6& o) {
    return h2j_out_opts8{o.scale_log2, o.max_dim, o.fit_w, o.fit_h, o.flags, o.crop_x, o.crop_y, o.crop_w, o.crop_h, o.orient,
                         o.qscale, o.sharpen, o.format, 0, 0, (o.reserved[0] | o.reserved[1] | o.reserved[2]) ? kColourReserved : 0};
}
h2j_out_opts8 widen8(const h2j_out_opts7& o) {
    return h2j_out_opts8{o.scale_log2, o.max_dim, o.fit_w, o.fit_h, o.flags, o.crop_x, o.crop_y, o.crop_w, o.crop_h, o.orient,
                         o.qscale, o.sharpen, o.format, o.pad, o.background, o.reserved[0] ? kColourReserved : 0};
}

bool reserved_zero(const h2j_out_opts6& o) { return std::all_of(o.reserved, o.reserved + 3, [](int32_t r) { return r == 0; }); }
bool reserved_zero(const h2j_out_opts8& o) { return o.colour != kColourReserved; }
// colour (include/h2j.h "Colour"): off, the stream's, or a source the caller names
bool colour_valid(const h2j_out_opts8& o) {
    if (o.colour == 0 || o.colour == H2J_COLOUR_AUTO) return true;
    const int mc = (o.colour & 0xFF) >> 1;
    return (o.colour & ~0xFF) == H2J_COLOUR_EXPLICIT && (mc == 1 || mc == 5 || mc == 6 || mc == 9);
}
// padded output (include/h2j.h "Padded output"): a two-sided box to pad to, a 24-bit colour, and no colour without pad
bool pad_valid(const h2j_out_opts8& o) {
    if (o.pad < 0 || o.pad > 1 || (o.background & ~0xFFFFFF)) return false;
    if (!o.pad) return o.background == 0;
    // (the canvas is the caller's number, not the picture's: H2J_PAD_MAX_SAMPLES bounds its memory and its int32 offsets)
    return o.fit_w >= 2 && o.fit_h >= 2 && static_cast<int64_t>(2 * (o.fit_w / 2)) * (2 * (o.fit_h / 2)) <= H2J_PAD_MAX_SAMPLES;
}
// finishing (include/h2j.h "Finishing"): a fixed quantiser scale, an unsharp mask
bool finish_valid(const h2j_out_opts8& o) { return (o.qscale == 0 || (o.qscale >= 2 && o.qscale <= 31)) && o.sharpen >= 0 && o.sharpen <= 64; }
// RGB output (include/h2j.h "RGB output"): a known format, and no quantiser scale for pixels
bool format_valid(const h2j_out_opts8& o) { return o.format >= H2J_FMT_JPEG && o.format <= H2J_FMT_RGB8_PLANAR && !(o.format && o.qscale); }
// the orientation (0, 2..8) the options name for a picture whose display orientation SEI says sei_orient
int resolve_orient(const h2j_out_opts8& o, int sei_orient) {
    const int r = o.orient == H2J_ORIENT_AUTO ? sei_orient : o.orient;
    return r == 1 ? 0 : r;
}
// Scaled output (include/h2j.h h2j_out_opts): the scale of a w x h picture -- scale_log2, or with
// max_dim > 0 the smallest k from scale_log2 up whose JPEG fits max_dim (3 if none does).
// Exact-size output (h2j_out_opts2): the size h2j_fit_size gives.
bool fit_valid(int fit_w, int fit_h, int flags) {
    return (fit_w == 0 || (fit_w >= 2 && fit_w <= 65535)) && (fit_h == 0 || (fit_h >= 2 && fit_h <= 65535)) &&
           (flags & ~H2J_FIT_STRETCH) == 0 && !((flags & H2J_FIT_STRETCH) && fit_w == 0 && fit_h == 0);
}
// what can be said of the options before the picture's size is known (an item none of whose renditions
// passes is not parsed); the window's place in the picture is checked by resolve_output
bool out_opts_valid(const h2j_out_opts8& o) {
    if (o.scale_log2 < 0 || o.scale_log2 > 3 || o.max_dim < 0) return false;
    if (!reserved_zero(o) || o.orient < H2J_ORIENT_AUTO || o.orient > 8 || !finish_valid(o) || !format_valid(o) || !pad_valid(o) || !colour_valid(o)) return false;
    if (o.crop_x < 0 || o.crop_y < 0 || o.crop_w < 0 || o.crop_h < 0 || ((o.crop_x | o.crop_y | o.crop_w | o.crop_h) & 1)) return false;
    if (o.flags & H2J_FIT_COVER) {  // a box, and nothing else that sizes the output
        if (o.flags != H2J_FIT_COVER || o.fit_w < 2 || o.fit_h < 2 || o.scale_log2 || o.max_dim) return false;
        return fit_valid(o.fit_w, o.fit_h, 0);
    }
    if (!fit_valid(o.fit_w, o.fit_h, o.flags)) return false;
    return !((o.fit_w || o.fit_h) && (o.scale_log2 || o.max_dim));
}
int resolve_scale(const h2j_out_opts8& o, int w, int h) {
    int k = o.scale_log2;
    if (o.max_dim > 0)
        while (k < 3 && std::max(h2j_scaled_dim(w, k), h2j_scaled_dim(h, k)) > o.max_dim) k++;
    return k;
}
// the output of a W x H picture (its parsed, cropped size) with options that passed out_opts_valid: the
// window (include/h2j.h "Crop and cover"; error H2J_ERR_OUT_OPTS if it does not lie in the picture), then
// what the remaining options make of a picture of the window's size.  A fit that resolves to the window's own
// size is the unscaled output; one that K3s makes on all three planes (w = ow 2^k, h = oh 2^k: the
// resampler's arithmetic reduces to K3s's there) is the scaled output of that k; K3r gets the rest.
// Orientation (include/h2j.h "Orientation"; sei_orient: the picture's, for H2J_ORIENT_AUTO) comes first: the
// rule runs on the oriented size, the window is in the oriented picture
static FrameJob::Output resolve_picture(const h2j_out_opts8& o, int W, int H, int sei_orient) {
    FrameJob::Output out;
    out.qscale = o.qscale;
    out.sharpen = o.sharpen;
    out.format = o.format;
    out.orient = resolve_orient(o, sei_orient);
    if (out.orient >= 5) std::swap(W, H);
    int64_t x = o.crop_x, y = o.crop_y, w = o.crop_w ? o.crop_w : W - x, h = o.crop_h ? o.crop_h : H - y;
    if (w < 2 || h < 2 || x + w > W || y + h > H) {
        out.error = H2J_ERR_OUT_OPTS;
        return out;
    }
    int fit_w = o.fit_w, fit_h = o.fit_h, flags = o.flags;
    if (flags & H2J_FIT_COVER) {  // the largest centred part of the window with the box's aspect, then a stretch
        const int64_t bw = fit_w, bh = fit_h;
        int64_t cw = w, ch = h;
        if (w * bh >= h * bw) cw = std::min(std::max<int64_t>(2 * ((h * bw) / (2 * bh)), 2), w);
        else ch = std::min(std::max<int64_t>(2 * ((w * bh) / (2 * bw)), 2), h);
        x += 2 * ((w - cw) / 4);
        y += 2 * ((h - ch) / 4);
        w = cw;
        h = ch;
        flags = H2J_FIT_STRETCH;
    }
    out.win_x = static_cast<int>(x);
    out.win_y = static_cast<int>(y);
    out.win_w = static_cast<int>(w);
    out.win_h = static_cast<int>(h);
    out.windowed = !(x == 0 && y == 0 && w == W && h == H);
    out.scale_log2 = resolve_scale(o, out.win_w, out.win_h);
    int ow = out.win_w, oh = out.win_h;
    if ((fit_w == 0 && fit_h == 0) || fit_size(out.win_w, out.win_h, fit_w, fit_h, flags, &ow, &oh) != 0) return out;
    if (ow == out.win_w && oh == out.win_h) return out;
    for (int k = 1; k <= 3; k++)
        if ((ow << k) == out.win_w && (oh << k) == out.win_h) {
            out.scale_log2 = k;
            return out;
        }
    out.scale_log2 = H2J_SCALE_RESAMPLE;
    out.fit_w = ow;
    out.fit_h = oh;
    return out;
}
// ... and the padding (include/h2j.h "Padded output") last: the picture part is what the options without pad resolve
// to, centred in the canvas the way cover centres its window; a picture part that fills the canvas is not padded
// The colour (include/h2j.h "Colour") is resolved with the picture: a source that is JFIF's already (BT.601, full range)
// leaves the output the one without the option
FrameJob::Output resolve_output(const h2j_out_opts8& o, int W, int H, int sei_orient, const int* stream_colour) {
    FrameJob::Output out = resolve_picture(o, W, H, sei_orient);
    if (out.error) return out;
    if (o.colour) {
        if (resolve_colour(o, stream_colour, &out.col_matrix, &out.col_full)) {
            out.error = H2J_ERR_OUT_OPTS;
            return out;
        }
        out.colour = (out.col_matrix == 6 && out.col_full) ? 0 : (H2J_COLOUR_EXPLICIT | out.col_matrix << 1 | out.col_full);
        if (out.colour) colour_coeffs(out.col_matrix, out.col_full, out.col_k);
    }
    if (!o.pad) return out;
    const int bw = 2 * (o.fit_w / 2), bh = 2 * (o.fit_h / 2), ow = out.out_w(), oh = out.out_h();
    if (ow == bw && oh == bh) return out;
    int ycc[3] = {0, 128, 128};
    pad_colour(static_cast<uint32_t>(o.background), ycc);
    out.pad = 1;
    out.box_w = bw;
    out.box_h = bh;
    out.pad_x = 2 * ((bw - ow) / 4);
    out.pad_y = 2 * ((bh - oh) / 4);
    for (int c = 0; c < 3; c++) out.fill[c] = static_cast<uint8_t>(ycc[c]);
    return out;
}
int resolve_colour(const h2j_out_opts8& o, const int* stream_colour, int* matrix, int* full) {
    int mc = 6, fr = 1;
    if (o.colour == H2J_COLOUR_AUTO) {
        mc = stream_colour ? stream_colour[2] : 2;
        fr = (stream_colour && stream_colour[3]) ? 1 : 0;  // (no range signalled: limited, E.2.1)
        if (mc == 2) mc = 6;  // unspecified: how the library reads such streams without the option
    } else if (o.colour != 0) {
        mc = (o.colour & 0xFF) >> 1;
        fr = o.colour & 1;
    }
    *matrix = mc == 5 ? 6 : mc;
    *full = fr;
    return (colour_valid(o) && (mc == 1 || mc == 5 || mc == 6 || mc == 9)) ? 0 : H2J_ERR_OUT_OPTS;
}

namespace {
// exact rationals on 128-bit integers (the terms below stay far inside them: denominators are products of a few
// four-digit numbers)
typedef __int128 I128;
struct Q {
    I128 n, d;  // d > 0, reduced
};
I128 gcd128(I128 a, I128 b) {
    if (a < 0) a = -a;
    while (b) {
        const I128 t = a % b;
        a = b;
        b = t;
    }
    return a ? a : 1;
}
Q mk(I128 n, I128 d) {
    if (d < 0) {
        n = -n;
        d = -d;
    }
    const I128 g = gcd128(n, d);
    return Q{n / g, d / g};
}
Q operator-(Q a, Q b) { return mk(a.n * b.d - b.n * a.d, a.d * b.d); }
Q operator*(Q a, Q b) { return mk(a.n * b.n, a.d * b.d); }
Q operator/(Q a, Q b) { return mk(a.n * b.d, a.d * b.n); }
// rnd(q 2^sh): to nearest, halves away from zero
int32_t rnd_shift(Q q, int sh) {
    const bool neg = q.n < 0;
    const I128 n = (neg ? -q.n : q.n) << sh;
    const I128 r = (2 * n + q.d) / (2 * q.d);
    return static_cast<int32_t>(neg ? -r : r);
}
}  // namespace

int colour_coeffs(int matrix, int full, int32_t* k) {
    if (!k || (full != 0 && full != 1) || !(matrix == 1 || matrix == 5 || matrix == 6 || matrix == 9)) return H2J_ERR_OUT_OPTS;
    const Q one = mk(1, 1), two = mk(2, 1);
    const Q Kr = matrix == 1 ? mk(2126, 10000) : matrix == 9 ? mk(2627, 10000) : mk(299, 1000);
    const Q Kb = matrix == 1 ? mk(722, 10000) : matrix == 9 ? mk(593, 10000) : mk(114, 1000);
    const Q Kg = one - Kr - Kb;
    const Q Krt = mk(299, 1000), Kbt = mk(114, 1000), Kgt = mk(587, 1000);  // the target: JFIF's
    const Q a = two * Kbt * (one - Kb) - two * Kgt * Kb * (one - Kb) / Kg;
    const Q b = two * Krt * (one - Kr) - two * Kgt * Kr * (one - Kr) / Kg;
    const Q c = (two * (one - Kb) - a) / (two * (one - Kbt));
    const Q d = (mk(0, 1) - b) / (two * (one - Kbt));
    const Q e = (mk(0, 1) - a) / (two * (one - Krt));
    const Q f = (two * (one - Kr) - b) / (two * (one - Krt));
    const Q g = mk(255, full ? 255 : 224);
    k[0] = full ? 0 : 16;
    k[1] = rnd_shift(mk(255, full ? 255 : 219), 20);
    k[2] = rnd_shift(a * g, 16);
    k[3] = rnd_shift(b * g, 16);
    k[4] = rnd_shift(c * g, 16);
    k[5] = rnd_shift(d * g, 16);
    k[6] = rnd_shift(e * g, 16);
    k[7] = rnd_shift(f * g, 16);
    return 0;
}

int pad_colour(uint32_t rgb, int* ycc) {
    if (!ycc || (rgb & ~0xFFFFFFu)) return H2J_ERR_OUT_OPTS;
    const int r = static_cast<int>(rgb >> 16), g = static_cast<int>((rgb >> 8) & 255), b = static_cast<int>(rgb & 255);
    auto clip = [](int v) { return v < 0 ? 0 : v > 255 ? 255 : v; };
    // JFIF's forward matrix in 16.16 (libjpeg's jccolor.c constants; >> of a negative int is arithmetic here)
    ycc[0] = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    ycc[1] = clip(((-11059 * r - 21709 * g + 32768 * b + 32768) >> 16) + 128);
    ycc[2] = clip(((32768 * r - 27439 * g - 5329 * b + 32768) >> 16) + 128);
    return 0;
}
// W, H: the parsed picture's cropped size (0: not parsed).  Options without a window or cover get the
// message they always got
std::string out_opts_message(const h2j_out_opts8& o, int W, int H, int sei_orient, const int* stream_colour) {
    std::string m = "invalid output options: scale_log2 " + std::to_string(o.scale_log2) + " (0..3), max_dim " +
           std::to_string(o.max_dim) + " (>= 0), fit " + std::to_string(o.fit_w) + " x " + std::to_string(o.fit_h) +
           " (0 or 2..65535, not with scale_log2 / max_dim), flags " + std::to_string(o.flags) +
           " (stretch needs a size), reserved " + (reserved_zero(o) ? "0" : "non-zero");
    const bool window = o.crop_x || o.crop_y || o.crop_w || o.crop_h || (o.flags & H2J_FIT_COVER);
    if (window)
        m += "; crop " + std::to_string(o.crop_x) + ", " + std::to_string(o.crop_y) + ", " + std::to_string(o.crop_w) + " x " +
             std::to_string(o.crop_h) + " (even, >= 0, at least 2 x 2 inside the picture; cover needs a box and excludes stretch, scale_log2, max_dim)";
    if (o.orient != 0) m += "; orient " + std::to_string(o.orient) + " (0..8, -1: the stream's display orientation)";
    if (o.qscale != 0 || o.sharpen != 0)
        m += "; qscale " + std::to_string(o.qscale) + " (0 or 2..31), sharpen " + std::to_string(o.sharpen) + " (0..64)";
    if (o.format != 0) m += "; format " + std::to_string(o.format) + " (0 JPEG, 1 RGB, 2 planar RGB; not with qscale)";
    if (o.pad != 0 || o.background != 0)
        m += "; pad " + std::to_string(o.pad) + " (0..1; needs a box: fit or cover with both sides, of at most " + std::to_string(H2J_PAD_MAX_SAMPLES) + " samples), background " + std::to_string(o.background) +
             " (0x00RRGGBB, 0 without pad)";
    if (o.colour != 0 && o.colour != kColourReserved) {
        m += "; colour " + std::to_string(o.colour) + " (0, -1: the stream's, or 256 | matrix_coefficients << 1 | full range with matrix_coefficients 1, 5, 6 or 9)";
        int mc = 0, fr = 0;
        if (o.colour == H2J_COLOUR_AUTO && W > 0 && H > 0 && resolve_colour(o, stream_colour, &mc, &fr))
            m += "; the stream signals matrix_coefficients " + std::to_string(mc) + ", which is not converted (1, 5, 6, 9 and 2 are)";
    }
    if (!(window && W > 0 && H > 0)) return m;
    const int ro = (o.orient >= H2J_ORIENT_AUTO && o.orient <= 8) ? resolve_orient(o, sei_orient) : 0;
    if (ro >= 5) std::swap(W, H);
    m += "; the picture is " + std::to_string(W) + " x " + std::to_string(H);
    if (ro) m += " at orientation " + std::to_string(ro);
    return m;
}

int crop_window6(int w, int h, const h2j_out_opts6* o, int sei_orient, int32_t* win, int* ow, int* oh, int* orient) {
    if (!o) return H2J_ERR_OUT_OPTS;
    const h2j_out_opts8 o8 = widen8(*o);  // (pad 0: the canvas is the picture part)
    int32_t place[4];
    return crop_window8(w, h, &o8, sei_orient, win, ow, oh, orient, place);
}

int crop_window7(int w, int h, const h2j_out_opts7* o, int sei_orient, int32_t* win, int* ow, int* oh, int* orient, int32_t* place) {
    if (!o) return H2J_ERR_OUT_OPTS;
    const h2j_out_opts8 o8 = widen8(*o);
    return crop_window8(w, h, &o8, sei_orient, win, ow, oh, orient, place);
}

int crop_window8(int w, int h, const h2j_out_opts8* o, int sei_orient, int32_t* win, int* ow, int* oh, int* orient, int32_t* place) {
    if (!o || !win || !ow || !oh || !orient || !place || w < 2 || h < 2 || w > 65536 || h > 65536 || ((w | h) & 1) || sei_orient < 0 ||
        sei_orient > 8 || !out_opts_valid(*o))
        return H2J_ERR_OUT_OPTS;
    const FrameJob::Output out = resolve_output(*o, w, h, sei_orient == 1 ? 0 : sei_orient);
    if (out.error) return out.error;
    *orient = out.orient;
    win[0] = out.win_x;
    win[1] = out.win_y;
    win[2] = out.win_w;
    win[3] = out.win_h;
    *ow = out.canvas_w();
    *oh = out.canvas_h();
    place[0] = out.pad_x;
    place[1] = out.pad_y;
    place[2] = out.out_w();
    place[3] = out.out_h();
    return 0;
}

int fit_size(int w, int h, int fit_w, int fit_h, int flags, int* ow, int* oh) {
    if (!ow || !oh || w < 2 || h < 2 || w > 65536 || h > 65536 || ((w | h) & 1) || !fit_valid(fit_w, fit_h, flags))
        return H2J_ERR_OUT_OPTS;
    const int64_t W = w, H = h;
    const int64_t bw = fit_w ? std::min<int64_t>(fit_w, W) : W, bh = fit_h ? std::min<int64_t>(fit_h, H) : H;
    int64_t wo, ho;
    if (flags & H2J_FIT_STRETCH) {
        wo = 2 * (bw / 2);
        ho = 2 * (bh / 2);
    } else if (bw * H <= bh * W) {  // the width binds
        wo = 2 * (bw / 2);
        ho = 2 * std::max<int64_t>(1, (H * wo) / (2 * W));
    } else {
        ho = 2 * (bh / 2);
        wo = 2 * std::max<int64_t>(1, (W * ho) / (2 * H));
    }
    *ow = static_cast<int>(wo);
    *oh = static_cast<int>(ho);
    return 0;
}

}  // namespace h2j
