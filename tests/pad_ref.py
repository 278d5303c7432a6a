"""Reference model of padded output (DESIGN.md "Padded output (K3b)") -- test infrastructure.

A padded rendition is its box: the picture part -- what the same options without `pad` resolve to, ow x oh, always
even and inside the box -- centred in a canvas BW x BH = 2 (fit_w / 2) x 2 (fit_h / 2) at

    px = 2 ((BW - ow) / 4),  py = 2 ((BH - oh) / 4)                   (all divisions floor)

the rest filled with one colour, JFIF's forward matrix in 16.16 on the background's R, G, B (arithmetic shifts):

    Y  = (19595 R + 38470 G +  7471 B + 32768) >> 16
    Cb = clip(((-11059 R - 21709 G + 32768 B + 32768) >> 16) + 128, 0, 255)
    Cr = clip((( 32768 R - 27439 G -  5329 B + 32768) >> 16) + 128, 0, 255)

The padded planes are 8-bit planes: Y (BH x BW) full of Y, Cb and Cr (BH/2 x BW/2) full of Cb, Cr, with the rendition's
final 8-bit planes written over the rectangle at (px, py) -- the chroma at (px / 2, py / 2).  Integer arithmetic only, so
GPU planes are compared byte for byte.
"""
import numpy as np


def pad_colour(rgb):
    """(R, G, B), each 0..255 -> the fill bytes (Y, Cb, Cr)."""
    r, g, b = (int(x) for x in rgb)
    assert all(0 <= x <= 255 for x in (r, g, b)), rgb
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16  # Python's >> on negative ints is arithmetic
    cb = ((-11059 * r - 21709 * g + 32768 * b + 32768) >> 16) + 128
    cr = ((32768 * r - 27439 * g - 5329 * b + 32768) >> 16) + 128
    return y, min(max(cb, 0), 255), min(max(cr, 0), 255)


def place(ow, oh, fit_w, fit_h):
    """(BW, BH, px, py) of an ow x oh picture part in the box fit_w x fit_h."""
    bw, bh = 2 * (fit_w // 2), 2 * (fit_h // 2)
    assert ow % 2 == 0 and oh % 2 == 0 and 2 <= ow <= bw and 2 <= oh <= bh, (ow, oh, fit_w, fit_h)
    return bw, bh, 2 * ((bw - ow) // 4), 2 * ((bh - oh) // 4)


def pad_planes(y, u, v, BW, BH, px, py, ycc):
    """8-bit planes of the picture part -> the padded planes Y (BH x BW), Cb, Cr (BH/2 x BW/2)."""
    y, u, v = np.asarray(y), np.asarray(u), np.asarray(v)
    h, w = y.shape
    assert y.dtype == u.dtype == v.dtype == np.uint8 and u.shape == v.shape == (h // 2, w // 2)
    assert BW % 2 == 0 and BH % 2 == 0 and px % 2 == 0 and py % 2 == 0 and 0 <= px and px + w <= BW and 0 <= py and py + h <= BH
    out = []
    for c, (p, sh) in enumerate(((y, 0), (u, 1), (v, 1))):
        canvas = np.full((BH >> sh, BW >> sh), ycc[c], dtype=np.uint8)
        canvas[py >> sh:(py >> sh) + p.shape[0], px >> sh:(px >> sh) + p.shape[1]] = p
        out.append(canvas)
    return tuple(out)
