"""Reference model of the exact-size JPEG output (DESIGN.md "Exact-size output (K3r)") -- test
infrastructure.

Integer arithmetic (int64 throughout) with one rounding, so GPU results are compared byte for
byte.  For a picture whose cropped output is W x H (4:2:0, both even):

* fit_size gives the output size W_o x H_o (even, never larger than the picture) of a fit box;
* each plane is resampled on its own grid, pw x ph -> ow x oh (ow <= pw, oh <= ph).  On a common
  grid of pw * ow units source column i covers [i ow, (i + 1) ow) and output column x covers
  [x pw, (x + 1) pw); the weight of i in x is the length of the overlap,
  wx = max(0, min((i + 1) ow, (x + 1) pw) - max(i ow, x pw)), rows likewise, and
  out = min(255, (2 S + D) // (2 D)) with S = sum wy wx p and D = pw ph 2^(bd - 8);
* the 8-bit planes go through the unchanged JPEG encoder (scale_ref.encode).
"""
import numpy as np

import oracle_py as O
import scale_ref as S

STRETCH = 1


def fit_size(w: int, h: int, fit, stretch: bool = False):
    """(W_o, H_o) of a cropped w x h picture for fit = (fit_w, fit_h), 0: no bound on that axis."""
    fw, fh = fit
    bw = min(fw, w) if fw else w
    bh = min(fh, h) if fh else h
    if stretch:
        return 2 * (bw // 2), 2 * (bh // 2)
    if bw * h <= bh * w:  # the width binds
        ow = 2 * (bw // 2)
        return ow, 2 * max(1, (h * ow) // (2 * w))
    oh = 2 * (bh // 2)
    return 2 * max(1, (w * oh) // (2 * h)), oh


def weights(pn: int, on: int) -> np.ndarray:
    """The dense on x pn weight matrix of one axis: row x holds the overlap of every source
    sample with output sample x (each row sums to pn, each column to on)."""
    i = np.arange(pn, dtype=np.int64)[None, :]
    x = np.arange(on, dtype=np.int64)[:, None]
    return np.maximum(0, np.minimum((i + 1) * on, (x + 1) * pn) - np.maximum(i * on, x * pn))


def _resample_axis1(g: np.ndarray, on: int) -> np.ndarray:
    """Unrounded weighted sums along axis 1 (pn -> on samples), tap by tap from the definition."""
    pn = g.shape[1]
    x = np.arange(on, dtype=np.int64)
    first = (x * pn) // on                      # first source sample output x overlaps
    taps = -(-pn // on) + 1                     # a footprint spans at most ceil(pn / on) + 1 samples
    out = np.zeros((g.shape[0], on), dtype=np.int64)
    for t in range(taps):
        i = first + t
        w = np.maximum(0, np.minimum((i + 1) * on, (x + 1) * pn) - np.maximum(i * on, x * pn))
        out += w[None, :] * g[:, np.minimum(i, pn - 1)]  # past the plane: weight 0
    return out


def area_plane(p: np.ndarray, bd: int, ow: int, oh: int) -> np.ndarray:
    """One cropped plane (2-D integer array, bit depth bd) -> its ow x oh uint8 plane."""
    ph, pw = p.shape
    assert 1 <= ow <= pw and 1 <= oh <= ph
    g = p.astype(np.int64)
    hs = _resample_axis1(g, ow)                 # < 2^29 per sample
    total = _resample_axis1(hs.T.copy(), oh).T  # < 2^59
    d = pw * ph * (1 << (bd - 8))
    return np.minimum((2 * total + d) // (2 * d), 255).astype(np.uint8)


def resize_planes(y, u, v, bd: int, ow: int, oh: int, bd_c=None):
    """Cropped Y, U, V planes of bit depth bd (chroma bd_c) -> the 8-bit planes of an ow x oh picture."""
    bd_c = bd if bd_c is None else bd_c
    assert ow % 2 == 0 and oh % 2 == 0
    return (area_plane(y, bd, ow, oh), area_plane(u, bd_c, ow // 2, oh // 2),
            area_plane(v, bd_c, ow // 2, oh // 2))


def expected(stream: bytes, codec: int, fit, stretch: bool = False):
    """(Y_o, U_o, V_o, JPEG bytes) the model expects for `stream` at fit / stretch; an output of
    the picture's own size is the oracle's unscaled transcode."""
    y, u, v, bd = O.decode(stream, codec)
    ow, oh = fit_size(y.shape[1], y.shape[0], fit, stretch)
    y8, u8, v8 = resize_planes(y, u, v, bd, ow, oh)
    same = (ow, oh) == (y.shape[1], y.shape[0])
    return y8, u8, v8, (O.transcode(stream) if same else S.encode(y8, u8, v8))
