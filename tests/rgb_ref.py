"""Reference model of RGB output (DESIGN.md "RGB output (K3c)") -- test infrastructure.

The source is a rendition's final 8-bit planes: Y (H x W) and Cb, Cr (H/2 x W/2), W and H even.  The chroma is
upsampled with JFIF's centred siting by the 9-3-3-1 triangle filter, kept at 16 x precision, and JFIF's (BT.601
full-range) matrix is applied in 16.16 fixed point with one rounding:

    cx = x >> 1,  nx = clamp(cx + ((x & 1) ? 1 : -1), 0, W/2 - 1);   cy, ny likewise with y, H/2
    C16(x, y) = 9 C[cy][cx] + 3 C[cy][nx] + 3 C[ny][cx] + C[ny][nx]          (0 .. 4080)
    db = Cb16 - 2048,  dr = Cr16 - 2048
    R = clip(((Y << 20) + 91881 dr                 + (1 << 19)) >> 20, 0, 255)
    G = clip(((Y << 20) - 22554 db - 46802 dr      + (1 << 19)) >> 20, 0, 255)
    B = clip(((Y << 20) + 116130 db                + (1 << 19)) >> 20, 0, 255)     (arithmetic shifts)

The model computes in int64 and asserts that every intermediate fits int32 (the GPU's type), so GPU pixels are
compared byte for byte.
"""
import numpy as np

KR, KGB, KGR, KB = 91881, 22554, 46802, 116130  # 1.402, 0.344136, 0.714136, 1.772 in 16.16
I32 = (-(1 << 31), (1 << 31) - 1)


def _i32(a):
    assert I32[0] <= int(a.min()) and int(a.max()) <= I32[1], (int(a.min()), int(a.max()))
    return a


def chroma16(c8):
    """An 8-bit chroma plane (H/2 x W/2) -> the 16 x upsampled plane (H x W), int64, 0 .. 4080."""
    c = np.asarray(c8).astype(np.int64)
    ch, cw = c.shape
    y, x = np.arange(2 * ch), np.arange(2 * cw)
    cy, cx = y >> 1, x >> 1
    ny = np.clip(cy + np.where(y & 1, 1, -1), 0, ch - 1)
    nx = np.clip(cx + np.where(x & 1, 1, -1), 0, cw - 1)
    out = 9 * c[np.ix_(cy, cx)] + 3 * c[np.ix_(cy, nx)] + 3 * c[np.ix_(ny, cx)] + c[np.ix_(ny, nx)]
    assert 0 <= int(out.min()) and int(out.max()) <= 4080
    return out


def rgb(y8, u8, v8):
    """8-bit 4:2:0 planes -> uint8 (H, W, 3) interleaved R, G, B."""
    y8, u8, v8 = np.asarray(y8), np.asarray(u8), np.asarray(v8)
    h, w = y8.shape
    assert h % 2 == 0 and w % 2 == 0 and u8.shape == v8.shape == (h // 2, w // 2), (y8.shape, u8.shape, v8.shape)
    assert y8.dtype == u8.dtype == v8.dtype == np.uint8
    yy = _i32((y8.astype(np.int64) << 20) + (1 << 19))
    db, dr = chroma16(u8) - 2048, chroma16(v8) - 2048
    r = _i32(yy + _i32(KR * dr)) >> 20  # numpy's >> on signed integers is arithmetic
    g = _i32(_i32(yy - _i32(KGB * db)) - _i32(KGR * dr)) >> 20
    b = _i32(yy + _i32(KB * db)) >> 20
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def rgb_planar(y8, u8, v8):
    """The same as uint8 (3, H, W): an R plane, a G plane, a B plane."""
    return np.ascontiguousarray(rgb(y8, u8, v8).transpose(2, 0, 1))


def convert(y8, u8, v8, fmt: str):
    """The pixels of format "rgb" or "rgb_planar"."""
    return {"rgb": rgb, "rgb_planar": rgb_planar}[fmt](y8, u8, v8)


def rgb_float(y8, u8, v8):
    """A float64 restatement: the same triangle weights, the real constants, round-half-up.  The integer model may
    differ from it by at most 1 (test_rgb_ref.py has the derivation)."""
    y = np.asarray(y8).astype(np.float64)
    db = chroma16(u8).astype(np.float64) / 16.0 - 128.0
    dr = chroma16(v8).astype(np.float64) / 16.0 - 128.0
    r = y + 1.402 * dr
    g = y - 0.344136 * db - 0.714136 * dr
    b = y + 1.772 * db
    return np.clip(np.floor(np.stack([r, g, b], axis=-1) + 0.5), 0, 255).astype(np.uint8)
