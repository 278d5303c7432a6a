"""The colour model (tests/colour_ref.py; DESIGN.md "Colour (K3v)") against its pins: the constants, the float64 and
scalar restatements, the range ends and the BT.709 bars -- and h2j_colour_coeffs, the host's integer computation of the
same constants."""
import ctypes

import numpy as np
import pytest

import colour_ref as COL
import h2j
import rgb_ref

# matrix, range -> oy, LY, LB, LR, CB, CR, RB, RR
TABLE = {
    ("bt601", "limited"): (16, 1220945, 0, 0, 74606, 0, 0, 74606),
    ("bt601", "full"): (0, 1048576, 0, 0, 65536, 0, 0, 65536),
    ("bt709", "limited"): (16, 1220945, 7578, 14628, 73849, -8255, -5405, 73367),
    ("bt709", "full"): (0, 1048576, 6657, 12850, 64871, -7252, -4748, 64448),
    ("bt2020", "limited"): (16, 1220945, 8795, 7872, 74248, -4443, -6273, 72854),
    ("bt2020", "full"): (0, 1048576, 7726, 6915, 65222, -3903, -5511, 63997),
}
SETS = sorted(TABLE)


def uniform(y, cb, cr):
    """2 x 2 pictures of one colour each, stacked: a (2 n) x 2 luma plane and n x 1 chroma planes would mix neighbours,
    so every colour is a picture of its own; returns lists of planes."""
    return (np.full((2, 2), y, np.uint8), np.full((1, 1), cb, np.uint8), np.full((1, 1), cr, np.uint8))


def one(y, cb, cr, matrix, rng):
    yo, uo, vo = COL.convert(*uniform(y, cb, cr), matrix, rng)
    assert len(set(yo.ravel().tolist())) == 1
    return int(yo[0, 0]), int(uo[0, 0]), int(vo[0, 0])


def test_the_constants_are_pinned():
    for key in SETS:
        assert COL.coeffs(*key) == TABLE[key], key
    # BT.601 full range is exactly the identity
    assert all(one(y, cb, cr, "bt601", "full") == (y, cb, cr) for y in (0, 1, 127, 254, 255) for cb in (0, 77, 255) for cr in (0, 200, 255))


@pytest.mark.parametrize("key", SETS)
def test_the_host_computes_the_same_constants(key):
    matrix, rng = key
    assert h2j.colour_coeffs(matrix, rng == "full") == TABLE[key]
    assert h2j.colour_coeffs(COL.MC[matrix], rng == "full") == TABLE[key]


def test_colour_coeffs_rejects_what_it_does_not_convert():
    lib = h2j.load_library()
    k = (ctypes.c_int32 * 8)(*[7] * 8)
    for mc, full in ((0, 0), (2, 0), (4, 1), (7, 0), (8, 0), (10, 1), (11, 0), (255, 0), (-1, 0), (1, 2), (1, -1)):
        assert lib.h2j_colour_coeffs(mc, full, k) == -60 and list(k) == [7] * 8, (mc, full)
    assert lib.h2j_colour_coeffs(1, 0, None) == -60
    assert h2j.colour_coeffs(5, False) == h2j.colour_coeffs(6, False) == TABLE[("bt601", "limited")]


def test_range_ends_and_the_709_bars():
    for matrix in ("bt601", "bt709", "bt2020"):
        assert one(16, 128, 128, matrix, "limited") == (0, 128, 128)
        assert one(235, 128, 128, matrix, "limited") == (255, 128, 128)
    assert one(63, 102, 240, "bt709", "limited") == (77, 85, 255)    # red
    assert one(173, 42, 26, "bt709", "limited") == (150, 44, 21)     # green
    assert one(32, 240, 118, "bt709", "limited") == (29, 255, 108)   # blue


@pytest.mark.parametrize("key", SETS)
def test_uniform_colours_against_float_and_scalar(key):
    """Y in 0..255, Cb and Cr stepped through 0, 3, ..., 255, as one picture per Cb: every Y (a pair of luma columns
    each) over chroma rows of one Cr each, every Cr three rows thick -- the middle row of a triple and its luma rows see
    uniform chroma, so the 9-3-3-1 filter changes nothing there; only those rows are compared."""
    matrix, rng = key
    steps = np.arange(0, 256, 3, dtype=np.uint8)
    n = len(steps)
    worst, big = 0.0, 0
    yy = np.repeat(np.arange(256, dtype=np.uint8), 2)[None, :].repeat(6 * n, 0)
    v = np.repeat(steps, 3)[:, None].repeat(256, 1)
    mid = 3 * np.arange(n) + 1                       # chroma rows with equal neighbours
    lmid = np.stack([2 * mid, 2 * mid + 1], 1).ravel()  # their luma rows
    for cb in steps:
        u = np.full((3 * n, 256), cb, np.uint8)
        got = COL.convert(yy, u, v, matrix, rng)
        flt = COL.convert_float(yy, u, v, matrix, rng)
        sums = COL.sums(yy, u, v, matrix, rng)
        for g, f, s, rows in zip(got, flt, sums, (lmid, mid, mid)):
            worst = max(worst, float(np.abs(g[rows].astype(np.float64) - np.clip(f[rows], 0, 255)).max()))
            big = max(big, int(np.abs(s[rows]).max()))
        if cb % 51 == 0:  # the scalar restatement, exactly
            for k in range(0, n, 17):
                cr = int(steps[k])
                for y in range(0, 256, 5):
                    want = COL.scalar(y, 16 * int(cb), 16 * cr, int(cb), cr, matrix, rng)
                    assert (int(got[0][2 * mid[k], 2 * y]), int(got[1][mid[k], y]), int(got[2][mid[k], y])) == want, (y, cb, cr)
    assert worst <= 1.0, worst   # (the largest seen: 0.501)
    assert big < 1 << 30, big    # int32 with room


def test_the_luma_reads_filtered_chroma():
    """Not uniform: the luma term takes K3c's 9-3-3-1 chroma at the luma position, the chroma planes no filter."""
    rng = np.random.default_rng(5)
    y = rng.integers(0, 256, (6, 10), dtype=np.uint8)
    u = rng.integers(0, 256, (3, 5), dtype=np.uint8)
    v = rng.integers(0, 256, (3, 5), dtype=np.uint8)
    yo, uo, vo = COL.convert(y, u, v, "bt709", "full")
    cb16, cr16 = rgb_ref.chroma16(u), rgb_ref.chroma16(v)
    for yy in range(6):
        for xx in range(10):
            want = COL.scalar(int(y[yy, xx]), int(cb16[yy, xx]), int(cr16[yy, xx]), int(u[yy >> 1, xx >> 1]), int(v[yy >> 1, xx >> 1]), "bt709", "full")
            assert (int(yo[yy, xx]), int(uo[yy >> 1, xx >> 1]), int(vo[yy >> 1, xx >> 1])) == want
