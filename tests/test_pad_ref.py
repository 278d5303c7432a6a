"""The model of padded output (tests/pad_ref.py) against restatements of its own rule: no engine, no GPU."""
import numpy as np

import pad_ref as PAD
import rgb_ref as RGB

COLOURS = [(r, g, b) for r in range(0, 256, 15) for g in range(0, 256, 15) for b in range(0, 256, 15)]
COLOURS += [(0, 0, 0), (255, 255, 255), (114, 114, 114), (255, 0, 16), (0, 0, 255), (255, 0, 0), (0, 255, 0), (1, 254, 3)]


def scalar(rgb):
    """The rule once more, with flooring divisions in place of the shifts."""
    r, g, b = rgb
    clip = lambda v: 0 if v < 0 else 255 if v > 255 else v
    return ((19595 * r + 38470 * g + 7471 * b + 32768) // 65536,
            clip((-11059 * r - 21709 * g + 32768 * b + 32768) // 65536 + 128),
            clip((32768 * r - 27439 * g - 5329 * b + 32768) // 65536 + 128))


def test_colour_matches_a_scalar_restatement():
    assert [PAD.pad_colour(c) for c in COLOURS] == [scalar(c) for c in COLOURS]
    # the rows of the matrix: the luma row sums to 1.0, the chroma rows to 0
    assert 19595 + 38470 + 7471 == 65536 and -11059 - 21709 + 32768 == 0 and 32768 - 27439 - 5329 == 0


def test_colour_is_within_one_of_float_jfif():
    # each 16.16 constant is within 2^-17 of JFIF's, so the sum before the rounding is within 3 * 255 * 2^-17 < 0.006 of
    # the real one: rounding it can move the result by at most 1 (and Cb, Cr of 255.5 clip to 255)
    for r, g, b in COLOURS:
        y = 0.299 * r + 0.587 * g + 0.114 * b
        cb = -0.168735892 * r - 0.331264108 * g + 0.5 * b + 128
        cr = 0.5 * r - 0.418687589 * g - 0.081312411 * b + 128
        got = PAD.pad_colour((r, g, b))
        for have, want in zip(got, (y, cb, cr)):
            assert abs(have - min(max(np.floor(want + 0.5), 0), 255)) <= 1, ((r, g, b), got, (y, cb, cr))


def test_greys_are_exact():
    for v in range(256):
        assert PAD.pad_colour((v, v, v)) == (v, 128, 128)
        px = RGB.rgb(*PAD.pad_planes(*(np.zeros(s, np.uint8) for s in ((2, 2), (1, 1), (1, 1))), 8, 8, 2, 2, (v, 128, 128)))
        assert (px[0, 0] == (v, v, v)).all()


def test_place_centres_as_cover_does():
    assert PAD.place(640, 360, 640, 640) == (640, 640, 0, 140)
    assert PAD.place(64, 64, 70, 66) == (70, 66, 2, 0) and PAD.place(64, 64, 78, 66) == (78, 66, 6, 0)
    assert PAD.place(64, 64, 91, 71) == (90, 70, 12, 2) and PAD.place(2, 16, 16, 16) == (16, 16, 6, 0)
    assert PAD.place(64, 64, 64, 64) == (64, 64, 0, 0) and PAD.place(64, 38, 100, 60) == (100, 60, 18, 10)
    for ow in range(2, 40, 2):
        for fit in range(ow, 44):
            bw, _, px, _ = PAD.place(ow, 2, fit, 2)
            assert bw == fit - fit % 2 and px % 2 == 0 and 0 <= px <= bw - ow - px <= px + 2


def test_planes_and_border():
    rng = np.random.default_rng(5)
    for (w, h, bw, bh), colour in zip(((64, 64, 90, 70), (2, 16, 16, 16), (6, 2, 6, 6), (24, 100, 46, 100), (64, 38, 100, 60)),
                                      ((114, 114, 114), (255, 0, 16), (0, 0, 0), (12, 200, 255), (255, 255, 255))):
        y, u, v = (rng.integers(0, 256, s, dtype=np.uint8) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2)))
        BW, BH, px, py = PAD.place(w, h, bw, bh)
        ycc = PAD.pad_colour(colour)
        Y, U, V = PAD.pad_planes(y, u, v, BW, BH, px, py, ycc)
        assert Y.shape == (BH, BW) and U.shape == V.shape == (BH // 2, BW // 2)
        assert np.array_equal(Y[py:py + h, px:px + w], y) and np.array_equal(U[py // 2:(py + h) // 2, px // 2:(px + w) // 2], u)
        assert np.array_equal(V[py // 2:(py + h) // 2, px // 2:(px + w) // 2], v)
        inside = np.zeros((BH, BW), bool)
        inside[py:py + h, px:px + w] = True
        assert (Y[~inside] == ycc[0]).all() and int((U == ycc[1]).sum()) >= U.size - u.size and int((V == ycc[2]).sum()) >= V.size - v.size
        # the RGB of the border, two or more pixels from the picture part (closer, the 9-3-3-1 filter mixes the picture's
        # chroma in, as it does in a viewer): the colour of a picture that is all border -- for a grey the colour itself;
        # else within 2: Y, Cb, Cr are each within 0.5 of the real value (1.0 where Cb or Cr clips at 255), which the
        # inverse matrix's largest row (1, 1.772) and its rounding turn into less than 0.5 + 1.772 + 0.5 < 3
        px8 = RGB.rgb(Y, U, V)
        far = np.ones((BH, BW), bool)
        far[max(py - 1, 0):py + h + 1, max(px - 1, 0):px + w + 1] = False
        flat = RGB.rgb(*(np.full(s, c, np.uint8) for s, c in (((2, 2), ycc[0]), ((1, 1), ycc[1]), ((1, 1), ycc[2]))))[0, 0]
        assert (px8[far] == flat).all()
        if colour[0] == colour[1] == colour[2]:
            assert tuple(int(c) for c in flat) == colour
        assert np.abs(flat.astype(int) - np.array(colour)).max() <= 2, (colour, flat)
