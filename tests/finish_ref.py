"""Reference model of the finishing options (DESIGN.md "Finishing (K3u, forced qscale)") -- test infrastructure.

sharpen: an unsharp mask on the 8-bit luma plane P (H x W), coordinates clamped to the plane:
    S(x, y) = sum of w[dy][dx] P(x + dx, y + dy), dy, dx in -1..1, w = [1 2 1; 2 4 2; 1 2 1]
    D = 16 P - S            out = clip(P + ((a D + 128) >> 8), 0, 255)       (arithmetic shift, a = 1..64)
Integer arithmetic with one rounding, so GPU planes are compared bit for bit.  The chroma is unchanged.

qscale: the JPEG of 8-bit planes at a quantiser scale the caller names instead of the rate control's.  The
quantiser is restated here in numpy on top of the oracle's own FDCT (oracle_fdct) and matrix
(oracle_jpeg_matrix), and the oracle's entropy coder and container (oracle_jpeg_from_coeffs) make the bytes.
test_finish_ref.py pins the restatement to oracle_jpeg_coeffs at the oracle's own qscale.
"""
import ctypes

import numpy as np

import oracle_py as O
import scale_ref as S

COM = S.COM

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48,
                   41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                   30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


def sharpen_planes(y8, u8, v8, a: int):
    """8-bit planes -> the planes with the luma through the unsharp mask of strength a / 16 (a = 0: unchanged)."""
    if a == 0:
        return y8, u8, v8
    p = np.pad(y8.astype(np.int32), 1, mode="edge")
    h, w = y8.shape
    s = np.zeros((h, w), dtype=np.int32)
    for dy, row in enumerate(((1, 2, 1), (2, 4, 2), (1, 2, 1))):
        for dx, k in enumerate(row):
            s += k * p[dy:dy + h, dx:dx + w]
    c = y8.astype(np.int32)
    d = 16 * c - s
    out = c + ((a * d + 128) >> 8)  # numpy's >> on signed integers is arithmetic
    return np.clip(out, 0, 255).astype(np.uint8), u8, v8


def matrix(q: int):
    """(M, q16, b16) of quantiser scale q: oracle_jpeg_matrix, natural order."""
    m, q16, b16 = (ctypes.c_uint8 * 64)(), (ctypes.c_uint16 * 64)(), (ctypes.c_uint16 * 64)()
    fn = O.lib().oracle_jpeg_matrix
    fn.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint16), ctypes.POINTER(ctypes.c_uint16)]
    fn.restype = None
    fn(int(q), m, q16, b16)
    return np.array(m[:], dtype=np.int64), np.array(q16[:], dtype=np.int64), np.array(b16[:], dtype=np.int64)


def _blocks(y8, u8, v8):
    """The 8 x 8 sample blocks of the padded picture (the last column / row replicated to whole
    MCUs), int16 [nmcu][6][64]: MCU raster, blocks Y00 Y01 Y10 Y11 Cb Cr."""
    h, w = y8.shape
    mbw, mbh = (w + 15) // 16, (h + 15) // 16

    def padded(p, pw, ph):
        ys = np.minimum(np.arange(ph), p.shape[0] - 1)
        xs = np.minimum(np.arange(pw), p.shape[1] - 1)
        return p.astype(np.int16)[np.ix_(ys, xs)]

    yp = padded(y8, mbw * 16, mbh * 16).reshape(mbh, 2, 8, mbw, 2, 8).transpose(0, 3, 1, 4, 2, 5).reshape(mbh * mbw, 4, 64)
    cp = [padded(c, mbw * 8, mbh * 8).reshape(mbh, 8, mbw, 8).transpose(0, 2, 1, 3).reshape(mbh * mbw, 1, 64) for c in (u8, v8)]
    return np.ascontiguousarray(np.concatenate([yp] + cp, axis=1))


def coeffs_q(y8, u8, v8, q: int):
    """Quantised zigzag coefficients int16 [nmcu][6][64] of 8-bit planes at quantiser scale q (2..31)."""
    blk = _blocks(y8, u8, v8)
    fdct = O.lib().oracle_fdct
    base, n = blk.ctypes.data, blk.shape[0] * 6
    for i in range(n):
        fdct(ctypes.cast(base + i * 128, ctypes.POINTER(ctypes.c_int16)))
    x = blk.reshape(n, 64).astype(np.int64)
    _, q16, b16 = matrix(q)
    a = np.abs(x)
    lv = np.minimum((np.minimum(a + b16, 65535) * q16) >> 16, 1023)
    nat = np.where(x < 0, -lv, lv)
    nat[:, 0] = ((x[:, 0] >> 2) + 8) // 16
    return nat[:, ZIGZAG].astype(np.int16).reshape(-1, 6, 64)


def encode_q(y8, u8, v8, q: int, com: bytes = COM) -> bytes:
    """The JPEG of 8-bit planes at quantiser scale q; q = 0: the rate control's (scale_ref.encode)."""
    if q == 0:
        return S.encode(y8, u8, v8, com)
    h, w = y8.shape
    return O.jpeg_from_coeffs(coeffs_q(y8, u8, v8, q), w, h, q, com)


def finish(y8, u8, v8, qscale: int = 0, sharpen: int = 0):
    """(Y, U, V, JPEG bytes) of a rendition whose unfinished 8-bit planes are y8, u8, v8: the sharpened planes are
    the picture, then the encoder at the forced scale or the rate control's."""
    p = sharpen_planes(y8, u8, v8, sharpen)
    return p[0], p[1], p[2], encode_q(p[0], p[1], p[2], qscale)
