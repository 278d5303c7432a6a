"""The numpy model of RGB output (tests/rgb_ref.py) against the definition (DESIGN.md "RGB output (K3c)"): a scalar
restatement straight from the formulas in Python integers, the cases the definition names, and a float64
restatement with the real constants."""
import numpy as np
import pytest

import rgb_ref as RGB


def scalar_rgb(y8, u8, v8):
    """The definition, one pixel at a time, in Python integers (unbounded: no overflow to hide)."""
    h, w = len(y8), len(y8[0])
    ch, cw = h // 2, w // 2
    clamp = lambda v, lo, hi: max(lo, min(hi, v))
    out = np.zeros((h, w, 3), dtype=np.uint8)
    for y in range(h):
        cy = y >> 1
        ny = clamp(cy + (1 if y & 1 else -1), 0, ch - 1)
        for x in range(w):
            cx = x >> 1
            nx = clamp(cx + (1 if x & 1 else -1), 0, cw - 1)
            c16 = [9 * int(c[cy][cx]) + 3 * int(c[cy][nx]) + 3 * int(c[ny][cx]) + int(c[ny][nx]) for c in (u8, v8)]
            db, dr = c16[0] - 2048, c16[1] - 2048
            yy = (int(y8[y][x]) << 20) + (1 << 19)
            for k, v in enumerate((yy + 91881 * dr, yy - 22554 * db - 46802 * dr, yy + 116130 * db)):
                assert abs(v) < 1 << 30
                out[y, x, k] = clamp(v >> 20, 0, 255)  # Python's >> floors: an arithmetic shift
    return out


def planes(rng, h, w, lo=0, hi=256):
    return (rng.integers(lo, hi, (h, w), dtype=np.uint8), rng.integers(lo, hi, (h // 2, w // 2), dtype=np.uint8),
            rng.integers(lo, hi, (h // 2, w // 2), dtype=np.uint8))


def test_constants_are_jfif_in_16_16():
    for k, real in ((RGB.KR, 1.402), (RGB.KGB, 0.344136), (RGB.KGR, 0.714136), (RGB.KB, 1.772)):
        # (22554 is the customary FIX(0.34414): 0.7 of a unit above 0.344136; the others are the nearest integers)
        assert abs(k - real * 65536) < 1 and abs(k / 65536 - real) <= 2.0 ** -16
    assert 255 * (1 << 20) + (1 << 19) + RGB.KB * 2048 < 1 << 30  # the largest magnitude: int32 holds it
    assert 255 * (1 << 20) + (1 << 19) + (RGB.KGB + RGB.KGR) * 2048 < 1 << 30


def test_grey_chroma_gives_grey():
    rng = np.random.default_rng(1)
    y = rng.integers(0, 256, (10, 14), dtype=np.uint8)
    y[0, :4] = (0, 1, 254, 255)
    c = np.full((5, 7), 128, dtype=np.uint8)
    out = RGB.rgb(y, c, c)
    for k in range(3):
        assert np.array_equal(out[:, :, k], y)


def test_2x2_every_clamp_hits_the_one_sample():
    y = np.array([[10, 200], [90, 255]], dtype=np.uint8)
    for cb, cr in ((128, 128), (0, 255), (255, 0), (77, 201), (16, 16), (240, 240)):
        u, v = np.array([[cb]], dtype=np.uint8), np.array([[cr]], dtype=np.uint8)
        assert int(RGB.chroma16(u)[1, 0]) == 16 * cb  # 9 + 3 + 3 + 1 times the one sample
        exp = np.zeros((2, 2, 3), dtype=np.uint8)
        for i in range(2):
            for j in range(2):
                yy, db, dr = (int(y[i, j]) << 20) + (1 << 19), 16 * cb - 2048, 16 * cr - 2048
                exp[i, j] = [max(0, min(255, t >> 20)) for t in (yy + 91881 * dr, yy - 22554 * db - 46802 * dr, yy + 116130 * db)]
        assert np.array_equal(RGB.rgb(y, u, v), exp), (cb, cr)
        assert np.array_equal(RGB.rgb(y, u, v), scalar_rgb(y, u, v))


def test_saturation_at_both_ends():
    hi = RGB.rgb(np.full((2, 2), 255, np.uint8), np.full((1, 1), 128, np.uint8), np.full((1, 1), 255, np.uint8))
    # Y 255, Cr 255: R clips at 255 (255 + 1.402 * 127), G = 255 - 0.714136 * 127 = 164.3, B = 255
    assert hi[0, 0].tolist() == [255, 164, 255] and (hi == hi[0, 0]).all()
    lo = RGB.rgb(np.zeros((2, 2), np.uint8), np.zeros((1, 1), np.uint8), np.full((1, 1), 128, np.uint8))
    # Y 0, Cb 0: B clips at 0 (-1.772 * 128), G = 0.344136 * 128 = 44.05, R = 0
    assert lo[0, 0].tolist() == [0, 44, 0] and (lo == lo[0, 0]).all()
    both = RGB.rgb(np.array([[255, 0], [0, 255]], np.uint8), np.array([[0]], np.uint8), np.array([[255]], np.uint8))
    assert both[0, 0].tolist() == [255, 208, 28] and both[0, 1].tolist() == [178, 0, 0]


def test_planar_is_the_transpose():
    y, u, v = planes(np.random.default_rng(2), 12, 18)
    a, b = RGB.rgb(y, u, v), RGB.rgb_planar(y, u, v)
    assert a.shape == (12, 18, 3) and b.shape == (3, 12, 18) and a.dtype == b.dtype == np.uint8
    assert np.array_equal(b, a.transpose(2, 0, 1)) and b.flags["C_CONTIGUOUS"]
    assert np.array_equal(RGB.convert(y, u, v, "rgb"), a) and np.array_equal(RGB.convert(y, u, v, "rgb_planar"), b)


@pytest.mark.parametrize("shape", [(2, 2), (2, 6), (6, 2), (4, 4), (10, 18), (16, 12)])
def test_model_is_the_definition(shape):
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    for lo, hi in ((0, 256), (0, 3), (253, 256)):
        y, u, v = planes(rng, *shape, lo=lo, hi=hi)
        assert np.array_equal(RGB.rgb(y, u, v), scalar_rgb(y, u, v)), (shape, lo, hi)


def test_model_against_float64_within_one():
    # The bound is derived, not measured: each 16.16 constant is within 2^-16 of the real one (all but 22554 within
    # 2^-17) and |d| / 16 <= 128, so a product differs from the real one by at most 128 * 2^-16 < 0.002 (G, two
    # products: < 0.004), and the triangle filter is exact in both.  The two values can therefore round to different
    # integers only when one lies within 0.004 of a rounding boundary, and then the integers are neighbours:
    # |difference| <= 1
    rng = np.random.default_rng(3)
    worst = 0
    for h, w in ((64, 64), (30, 52), (2, 2), (128, 96)):
        y, u, v = planes(rng, h, w)
        d = np.abs(RGB.rgb(y, u, v).astype(np.int32) - RGB.rgb_float(y, u, v).astype(np.int32))
        worst = max(worst, int(d.max()))
        assert (d > 0).mean() < 0.01  # ... and a pixel near a boundary is rare
    assert worst <= 1


def test_rejects_bad_shapes():
    with pytest.raises(AssertionError):
        RGB.rgb(np.zeros((3, 4), np.uint8), np.zeros((1, 2), np.uint8), np.zeros((1, 2), np.uint8))
    with pytest.raises(AssertionError):
        RGB.rgb(np.zeros((4, 4), np.uint8), np.zeros((2, 2), np.uint8), np.zeros((2, 1), np.uint8))
    with pytest.raises(AssertionError):
        RGB.rgb(np.zeros((4, 4), np.uint16), np.zeros((2, 2), np.uint8), np.zeros((2, 2), np.uint8))
