"""Reference model of the scaled JPEG output (DESIGN.md "Scaled output") -- test infrastructure.

Integer arithmetic with one rounding, so GPU results are compared byte for byte.  For a
picture whose cropped output is W x H (4:2:0, both even) at scale k (factor s = 1 << k):

* scaled chroma size cw = ceil(W / 2s), ch = ceil(H / 2s); scaled luma size W_k = 2 cw,
  H_k = 2 ch (always even); k = 0 gives W x H;
* each plane on its own grid: output sample (x, y) of a plane of bit depth bd is
  min(255, (S + (1 << (sh - 1))) >> sh) with sh = 2k + bd - 8, S the sum of the s x s source
  samples at (x s + i, y s + j) of the cropped plane, coordinates clamped to its last column /
  row; at sh = 0 the sample is copied (k = 0 is the 10 -> 8 bit rule of oracle/transcode_ref.c);
* the scaled 8-bit planes go through the unchanged JPEG encoder: the expected bytes are
  oracle_jpeg_encode(Y_k, U_k, V_k, W_k, H_k, W_k, W_k / 2, "Lavc58.117.101").
"""
import ctypes

import numpy as np

import oracle_py as O

COM = b"Lavc58.117.101"


def scaled_size(w: int, h: int, k: int):
    """(W_k, H_k) of a W x H picture at scale k."""
    s = 1 << k
    cw, ch = -(-w // (2 * s)), -(-h // (2 * s))
    return 2 * cw, 2 * ch


def resolve_scale(w: int, h: int, scale: int = 0, max_dim: int = 0) -> int:
    """The max_dim rule: the smallest k in [scale, 3] with max(W_k, H_k) <= max_dim; 3 if none fits."""
    k = scale
    if max_dim > 0:
        while k < 3 and max(scaled_size(w, h, k)) > max_dim:
            k += 1
    return k


def box_plane(p: np.ndarray, bd: int, k: int, ow: int, oh: int) -> np.ndarray:
    """One cropped plane (2-D integer array, bit depth bd) -> its ow x oh uint8 plane at scale k."""
    s = 1 << k
    ys = np.minimum(np.arange(oh * s), p.shape[0] - 1)
    xs = np.minimum(np.arange(ow * s), p.shape[1] - 1)
    g = p.astype(np.int64)[np.ix_(ys, xs)]
    total = g.reshape(oh, s, ow, s).sum(axis=(1, 3))
    sh = 2 * k + bd - 8
    out = total if sh == 0 else (total + (1 << (sh - 1))) >> sh
    return np.minimum(out, 255).astype(np.uint8)


def scale_planes(y, u, v, bd: int, k: int, bd_c=None):
    """Cropped Y, U, V planes of bit depth bd (chroma bd_c) -> the 8-bit planes at scale k."""
    bd_c = bd if bd_c is None else bd_c
    wk, hk = scaled_size(y.shape[1], y.shape[0], k)
    return (box_plane(y, bd, k, wk, hk), box_plane(u, bd_c, k, wk // 2, hk // 2),
            box_plane(v, bd_c, k, wk // 2, hk // 2))


def encode(y8, u8, v8, com: bytes = COM) -> bytes:
    """oracle_jpeg_encode of 8-bit planes (luma W_k x H_k, chroma half of it, contiguous rows)."""
    h, w = y8.shape
    assert u8.shape == (h // 2, w // 2) and v8.shape == u8.shape
    planes = [np.ascontiguousarray(a, dtype=np.uint8) for a in (y8, u8, v8)]
    p = [a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)) for a in planes]
    cap = w * h * 4 + (1 << 20)
    out = (ctypes.c_uint8 * cap)()
    n = O.lib().oracle_jpeg_encode(p[0], p[1], p[2], w, h, w, w // 2, com, out, cap)
    if n <= 0:
        raise RuntimeError(f"oracle_jpeg_encode failed {n}")
    return bytes(out[:n])


def codec_of(path: str) -> int:
    return 264 if path.endswith(".h264") else 265


def expected(stream: bytes, codec: int, k: int):
    """(Y_k, U_k, V_k, JPEG bytes) the model expects for `stream` at scale k."""
    y, u, v, bd = O.decode(stream, codec)
    y8, u8, v8 = scale_planes(y, u, v, bd, k)
    return y8, u8, v8, encode(y8, u8, v8)
