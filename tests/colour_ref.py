"""Reference model of colour (DESIGN.md "Colour (K3v)") -- test infrastructure.

The source is a rendition's 8-bit planes after orientation, window and scale / fit: Y (H x W) and Cb, Cr (H/2 x W/2), W
and H even, in the source's matrix m and range.  The result is the same picture in JFIF's: BT.601, full range.

    matrix   (Kr, Kb):  bt601 (0.299, 0.114)   bt709 (0.2126, 0.0722)   bt2020 (0.2627, 0.0593), non-constant luminance
    range    (oy, sy, sc):  limited (16, 219, 224)   full (0, 255, 255)

With Kg = 1 - Kr - Kb and the target Kr' = 0.299, Kb' = 0.114, Kg' = 0.587, in exact rationals:

    a = 2 Kb'(1-Kb) - 2 Kg' Kb (1-Kb)/Kg        b = 2 Kr'(1-Kr) - 2 Kg' Kr (1-Kr)/Kg
    c = (2(1-Kb) - a) / (2(1-Kb'))              d = -b / (2(1-Kb'))
    e = -a / (2(1-Kr'))                         f = (2(1-Kr) - b) / (2(1-Kr'))
    g = 255 / sc
    LY = rnd(255/sy 2^20)   LB = rnd(a g 2^16)   LR = rnd(b g 2^16)
    CB = rnd(c g 2^16)      CR = rnd(d g 2^16)   RB = rnd(e g 2^16)   RR = rnd(f g 2^16)

(rnd: to nearest, halves away from zero).  Where they come from: Y' = Kr' R + Kg' G + Kb' B of the R, G, B the source's
Y, Pb, Pr stand for is Y + a Pb + b Pr, and Pb' = (B - Y') / (2 (1 - Kb')), Pr' = (R - Y') / (2 (1 - Kr')) give c .. f.
With Cb16, Cr16 K3c's 9-3-3-1 chroma at luma position (x, y), 16 x precision (rgb_ref.chroma16):

    Y'(x, y)  = clip((LY (Y - oy) + LB (Cb16 - 2048) + LR (Cr16 - 2048) + 2^19) >> 20, 0, 255)
    Cb'(i, j) = clip((CB (Cb - 128) + CR (Cr - 128) + (128 << 16) + 2^15) >> 16, 0, 255)
    Cr'(i, j) = clip((RB (Cb - 128) + RR (Cr - 128) + (128 << 16) + 2^15) >> 16, 0, 255)

All shifts arithmetic; chroma is converted at chroma positions, with no filter.  The model computes in int64 and asserts
that every intermediate fits int32 (the GPU's type), so GPU planes are compared byte for byte.
"""
from fractions import Fraction as F

import numpy as np

import rgb_ref

MATRICES = {"bt601": (F(299, 1000), F(114, 1000)), "bt709": (F(2126, 10000), F(722, 10000)), "bt2020": (F(2627, 10000), F(593, 10000))}
RANGES = {"limited": (16, 219, 224), "full": (0, 255, 255)}
MC = {"bt601": 6, "bt709": 1, "bt2020": 9}  # matrix_coefficients of each name (5 is bt601 too)
MC_NAME = {1: "bt709", 5: "bt601", 6: "bt601", 9: "bt2020", 2: "bt601"}
I32 = (-(1 << 31), (1 << 31) - 1)


def _i32(a):
    assert I32[0] <= int(np.min(a)) and int(np.max(a)) <= I32[1], (int(np.min(a)), int(np.max(a)))
    return a


def rnd(q):
    """A Fraction to the nearest integer, halves away from zero."""
    n = (2 * abs(q.numerator) + q.denominator) // (2 * q.denominator)
    return -n if q < 0 else n


def rationals(matrix):
    """a .. f of the source matrix, exact."""
    kr, kb = MATRICES[matrix]
    kg = 1 - kr - kb
    krt, kbt = MATRICES["bt601"]
    kgt = 1 - krt - kbt
    a = 2 * kbt * (1 - kb) - 2 * kgt * kb * (1 - kb) / kg
    b = 2 * krt * (1 - kr) - 2 * kgt * kr * (1 - kr) / kg
    c = (2 * (1 - kb) - a) / (2 * (1 - kbt))
    d = -b / (2 * (1 - kbt))
    e = -a / (2 * (1 - krt))
    f = (2 * (1 - kr) - b) / (2 * (1 - krt))
    return a, b, c, d, e, f


def coeffs(matrix, rng):
    """(oy, LY, LB, LR, CB, CR, RB, RR) of a source matrix and range."""
    oy, sy, sc = RANGES[rng]
    a, b, c, d, e, f = rationals(matrix)
    g = F(255, sc)
    return (oy, rnd(F(255, sy) * (1 << 20)), rnd(a * g * (1 << 16)), rnd(b * g * (1 << 16)), rnd(c * g * (1 << 16)),
            rnd(d * g * (1 << 16)), rnd(e * g * (1 << 16)), rnd(f * g * (1 << 16)))


def word(matrix, rng):
    """The C encoding of an explicit colour: H2J_COLOUR_EXPLICIT | mc << 1 | full."""
    return 0x100 | MC[matrix] << 1 | (1 if rng == "full" else 0)


def sums(y8, u8, v8, matrix, rng):
    """The three accumulators before their shift, int64 (what the clips act on)."""
    y8, u8, v8 = np.asarray(y8), np.asarray(u8), np.asarray(v8)
    h, w = y8.shape
    assert h % 2 == 0 and w % 2 == 0 and u8.shape == v8.shape == (h // 2, w // 2), (y8.shape, u8.shape, v8.shape)
    assert y8.dtype == u8.dtype == v8.dtype == np.uint8
    oy, LY, LB, LR, CB, CR, RB, RR = coeffs(matrix, rng)
    db16, dr16 = rgb_ref.chroma16(u8) - 2048, rgb_ref.chroma16(v8) - 2048
    sy = _i32(_i32(_i32(LY * (y8.astype(np.int64) - oy)) + _i32(LB * db16)) + _i32(LR * dr16)) + (1 << 19)
    db, dr = u8.astype(np.int64) - 128, v8.astype(np.int64) - 128
    su = _i32(_i32(CB * db) + _i32(CR * dr)) + (128 << 16) + (1 << 15)
    sv = _i32(_i32(RB * db) + _i32(RR * dr)) + (128 << 16) + (1 << 15)
    return _i32(sy), _i32(su), _i32(sv)


def convert(y8, u8, v8, matrix, rng):
    """8-bit 4:2:0 planes in (matrix, range) -> the normalised 8-bit planes (Y', Cb', Cr')."""
    sy, su, sv = sums(y8, u8, v8, matrix, rng)
    clip = lambda a: np.clip(a, 0, 255).astype(np.uint8)  # noqa: E731  (numpy's >> on signed integers is arithmetic)
    return clip(sy >> 20), clip(su >> 16), clip(sv >> 16)


def convert_float(y8, u8, v8, matrix, rng):
    """A float64 restatement with the real constants and round-half-up: the integer model stays within 1 of it."""
    oy, sy, sc = RANGES[rng]
    a, b, c, d, e, f = (float(x) for x in rationals(matrix))
    y = (np.asarray(y8).astype(np.float64) - oy) * 255.0 / sy
    g = 255.0 / sc
    pb = (rgb_ref.chroma16(u8).astype(np.float64) / 16.0 - 128.0) * g
    pr = (rgb_ref.chroma16(v8).astype(np.float64) / 16.0 - 128.0) * g
    cb, cr = (np.asarray(u8).astype(np.float64) - 128.0) * g, (np.asarray(v8).astype(np.float64) - 128.0) * g
    return y + a * pb + b * pr, 128.0 + c * cb + d * cr, 128.0 + e * cb + f * cr


def scalar(Y, cb16, cr16, cb, cr, matrix, rng):
    """One luma sample (from its 16 x chroma) and one chroma pair, in plain Python integers."""
    oy, LY, LB, LR, CB, CR, RB, RR = coeffs(matrix, rng)
    clip = lambda v: max(0, min(255, v))  # noqa: E731
    yo = clip((LY * (Y - oy) + LB * (cb16 - 2048) + LR * (cr16 - 2048) + (1 << 19)) >> 20)
    uo = clip((CB * (cb - 128) + CR * (cr - 128) + (128 << 16) + (1 << 15)) >> 16)
    vo = clip((RB * (cb - 128) + RR * (cr - 128) + (128 << 16) + (1 << 15)) >> 16)
    return yo, uo, vo
