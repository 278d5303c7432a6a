"""The reference model of the exact-size JPEG output (tests/resize_ref.py): its reduction to the
box filter of tests/scale_ref.py, hand cases, the size rule -- the model's and the library's
h2j_fit_size -- and the public symbols of the feature (no GPU needed)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import resize_ref as R
import scale_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "h264-h265-to-jpeg_amd")

# (source, fit, output): the worked values of the size rule
TABLE = [
    ((1920, 1080), (512, 512), (512, 288)),
    ((1920, 1080), (100, 100), (100, 56)),
    ((1920, 1080), (500, 0), (500, 280)),
    ((1920, 1080), (1280, 720), (1280, 720)),
    ((72, 40), (50, 0), (50, 26)),
    ((48, 200), (16, 16), (2, 16)),
    ((64, 64), (2, 2), (2, 2)),
]


def sweep():
    """10,000 seeded (w, h, fit, stretch) tuples: sizes to 8192, boxes to 65535, zeros included."""
    rng = np.random.default_rng(20261019)
    out = []
    for _ in range(10000):
        hi = int(rng.choice([64, 512, 4096]))
        w, h = 2 * int(rng.integers(1, hi + 1)), 2 * int(rng.integers(1, hi + 1))
        fit = []
        for n in (w, h):
            kind = int(rng.integers(0, 5))
            fit.append(0 if kind == 0 else int(rng.integers(2, 65536)) if kind == 1 else int(rng.integers(2, n + 3)))
        stretch = bool(rng.integers(0, 2)) and (fit[0] or fit[1])
        out.append((w, h, tuple(fit), bool(stretch)))
    return out


@pytest.mark.parametrize("bd", [8, 10, 14])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_area_equals_box_at_divisible_sizes(bd, k):
    rng = np.random.default_rng(100 * bd + k)
    for ow, oh in ((5, 3), (16, 8), (1, 7)):
        p = rng.integers(0, 1 << bd, size=(oh << k, ow << k)).astype(np.uint16)
        assert np.array_equal(R.area_plane(p, bd, ow, oh), S.box_plane(p, bd, k, ow, oh)), (ow, oh)


@pytest.mark.parametrize("pn,on", [(64, 62), (64, 34), (72, 50), (1080, 720), (1920, 512), (540, 8), (7, 7), (9, 1)])
def test_weights_sum_to_the_source_and_output_lengths(pn, on):
    w = R.weights(pn, on)
    assert (w.sum(axis=1) == pn).all()   # every output sample: pw (ph) units
    assert (w.sum(axis=0) == on).all()   # every source sample is used exactly once: ow (oh) units
    assert ((w > 0).sum(axis=0) <= 2).all()  # on <= pn: a source sample overlaps at most two outputs


@pytest.mark.parametrize("pn,on", [(102, 100), (150, 100), (188, 100), (320, 10)])  # 1.02, 1.5, 1.88, 32
def test_constant_plane_stays_constant(pn, on):
    for bd, val in ((8, 0), (8, 1), (8, 77), (8, 255), (10, 4 * 77), (10, 4 * 77 + 1), (12, 16 * 200)):
        p = np.full((pn, pn + 2), val, dtype=np.uint16)
        e = min(255, (val + ((1 << (bd - 8)) >> 1)) >> (bd - 8))
        assert (R.area_plane(p, bd, on, on) == e).all(), (bd, val)
        assert (R.area_plane(p, bd, pn + 2, on) == e).all(), (bd, val)  # one axis at ratio 1


def test_all_maximum_10_bit_plane_gives_255():
    p = np.full((30, 46), 1023, dtype=np.uint16)
    d = 30 * 46 * 4
    assert (2 * 1023 * 30 * 46 + d) // (2 * d) == 256  # before the clamp
    assert (R.area_plane(p, 10, 31, 7) == 255).all()


def test_hand_case_three_to_two():
    p = np.array([[10, 20, 40]], dtype=np.uint16)  # weights (2, 1, 0) and (0, 1, 2), D = 3
    assert R.area_plane(p, 8, 2, 1).tolist() == [[(2 * (2 * 10 + 20) + 3) // 6, (2 * (20 + 2 * 40) + 3) // 6]]


@pytest.mark.parametrize("src,fit,out", TABLE)
def test_fit_size_table(src, fit, out):
    assert R.fit_size(src[0], src[1], fit) == out


def check_properties(size_fn):
    for w, h, fit, stretch in sweep():
        ow, oh = size_fn(w, h, fit, stretch)
        t = (w, h, fit, stretch, ow, oh)
        assert ow >= 2 and oh >= 2 and ow % 2 == 0 and oh % 2 == 0, t
        assert ow <= w and oh <= h, t
        assert (not fit[0] or ow <= fit[0]) and (not fit[1] or oh <= fit[1]), t
        if (not fit[0] or fit[0] >= w) and (not fit[1] or fit[1] >= h):
            assert (ow, oh) == (w, h), t
        if stretch:
            assert ow == 2 * (min(fit[0] or w, w) // 2) and oh == 2 * (min(fit[1] or h, h) // 2), t
        else:  # one axis takes its bound, the other keeps the aspect (floored to even, at least 2)
            assert ow == 2 * (min(fit[0] or w, w) // 2) or oh == 2 * (min(fit[1] or h, h) // 2), t


def test_fit_size_properties():
    check_properties(R.fit_size)
    assert R.fit_size(1920, 1080, (500, 100), True) == (500, 100)
    assert R.fit_size(1920, 1080, (0, 101), True) == (1920, 100)
    assert R.fit_size(8192, 2, (65535, 0)) == (8192, 2)


def test_library_fit_size_agrees_with_the_model():
    import h2j
    for src, fit, out in TABLE:
        assert h2j.fit_size(src[0], src[1], fit) == out
    check_properties(h2j.fit_size)
    for w, h, fit, stretch in sweep():
        assert h2j.fit_size(w, h, fit, stretch) == R.fit_size(w, h, fit, stretch), (w, h, fit, stretch)
    assert h2j.fit_size(1920, 1080, (None, 720)) == (1280, 720)
    lib = h2j.load_library()
    ow, oh = ctypes.c_int(-7), ctypes.c_int(-7)
    for args in ((64, 64, 1, 0, 0), (64, 64, 0, -2, 0), (64, 64, 65536, 0, 0), (64, 64, 8, 8, 2), (64, 64, 0, 0, 1)):
        assert lib.h2j_fit_size(*args, ctypes.byref(ow), ctypes.byref(oh)) == h2j.ERR_OUT_OPTS, args
        assert (ow.value, oh.value) == (-7, -7)


def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(h2j_[a-z0-9_]+)\s*\(", src))


def _exports(so):
    path = os.path.join(PKG, so)
    if not os.path.exists(path):
        subprocess.check_call(["make", "-s", "-C", PKG])
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_exact_size_symbols_declared_and_exported():
    host = {"h2j_engine_submit_opts2", "h2j_engine_transcode_opts2", "h2j_engine_decode_resized",
            "h2j_h265_to_jpeg_mem_fit", "h2j_fit_size"}
    assert host <= _declared("h2j.h")
    assert host <= _exports("libH265ToJpeg.so")
    # the v1 entry points stay
    assert {"h2j_engine_submit_opts", "h2j_engine_transcode_opts", "h2j_h265_to_jpeg_mem_scaled",
            "h2j_engine_decode_scaled"} <= _exports("libH265ToJpeg.so")


def test_option_struct_layouts():
    import h2j
    assert ctypes.sizeof(h2j.OutOpts) == 8       # h2j_out_opts is unchanged
    assert ctypes.sizeof(h2j.OutOpts2) == 32
    assert h2j.OutOpts2.fit_w.offset == 8 and h2j.OutOpts2.flags.offset == 16 and h2j.OutOpts2.reserved.offset == 20
