"""The finishing model (tests/finish_ref.py) against the oracle, without a GPU: the quantiser restated there is
the oracle's at the oracle's own quantiser scale, before anything is compared with the GPU; and the unsharp mask's
arithmetic on planes small enough to check by hand."""
import numpy as np
import pytest

import finish_ref as F
import oracle_py as O
import scale_ref as S
from conftest import golden, read

VECTORS = ["img01.h265", "hevc/p12_72x40_odd_crop.h265", "hevc/p11_64x64_tiny.h265"]


@pytest.mark.parametrize("name", VECTORS)
def test_restated_quantiser_is_the_oracles(name):
    y, u, v, bd = O.decode(read(golden(name)), S.codec_of(name))
    y8, u8, v8 = (O.to8(p, bd) for p in (y, u, v))
    q, want = O.jpeg_coeffs(y8, u8, v8)
    assert 2 <= q <= 31
    got = F.coeffs_q(y8, u8, v8, q)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert F.encode_q(y8, u8, v8, q) == S.encode(y8, u8, v8)
    assert F.encode_q(y8, u8, v8, 0) == S.encode(y8, u8, v8)


def test_other_scales_differ_and_order():
    y, u, v, bd = O.decode(read(golden(VECTORS[1])), 265)
    sizes = [len(F.encode_q(y, u, v, q)) for q in (2, 8, 31)]
    assert sizes[0] > sizes[1] > sizes[2]
    m2, m31 = F.matrix(2)[0], F.matrix(31)[0]
    assert m2[0] == m31[0] == 8 and m2[1] == (16 * 2) >> 3 and m31[63] == min(255, (83 * 31) >> 3)


def test_sharpen_arithmetic():
    flat = np.full((6, 8), 77, dtype=np.uint8)
    c = np.zeros((3, 4), dtype=np.uint8)
    for a in (1, 16, 64):
        assert np.array_equal(F.sharpen_planes(flat, c, c, a)[0], flat)  # D = 0 on a flat plane, edges included
    # one bright sample in a dark plane: S = 4 * 100 at it, 2 * 100 beside it, 100 diagonally
    p = np.zeros((5, 5), dtype=np.uint8)
    p[2, 2] = 100
    out = F.sharpen_planes(p, c, c, 16)[0]
    assert out[2, 2] == 100 + ((16 * (1600 - 400) + 128) >> 8) == 175
    assert out[2, 1] == 0 and out[1, 1] == 0  # 0 + ((16 * -200 + 128) >> 8) = -12, clipped
    assert F.sharpen_planes(p, c, c, 64)[0][2, 2] == 255  # 100 + 300, clipped
    # the arithmetic shift rounds towards minus infinity: a = 1, D = -200: (-200 + 128) >> 8 = -1
    q = np.full((5, 5), 50, dtype=np.uint8)
    q[2, 2] = 150
    assert F.sharpen_planes(q, c, c, 1)[0][2, 1] == 50 + ((1 * (16 * 50 - (16 * 50 + 200)) + 128) >> 8) == 49
    # clamped coordinates: a corner sample counts 9 / 16 in its own S
    r = np.zeros((4, 4), dtype=np.uint8)
    r[0, 0] = 160
    assert F.sharpen_planes(r, c, c, 16)[0][0, 0] == 160 + ((16 * (2560 - 9 * 160) + 128) >> 8) == 230
    # a 2 x 2 plane: both clamps hit the same sample
    t = np.array([[10, 200], [90, 30]], dtype=np.uint8)
    s00 = 9 * 10 + 3 * 200 + 3 * 90 + 30
    assert F.sharpen_planes(t, c[:1, :1], c[:1, :1], 32)[0][0, 0] == max(0, 10 + ((32 * (160 - s00) + 128) >> 8))
    y, u, v = F.sharpen_planes(t, c, c, 0)
    assert y is t and u is c
