"""The reference model of the scaled JPEG output (tests/scale_ref.py): hand cases, the model
pinned to the oracle at k = 0, and the public symbols of the feature (no GPU needed)."""
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_py as O
import scale_ref as R
from conftest import golden, read

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "h264-h265-to-jpeg_amd")


def test_box_rounds_half_up():
    p = np.array([[0, 1], [1, 1]], dtype=np.uint16)
    assert R.box_plane(p, 8, 1, 1, 1).tolist() == [[1]]  # (3 + 2) >> 2


def test_clamp_is_live_at_10_bits():
    p = np.full((2, 2), 1023, dtype=np.uint16)
    # sh = 4: (4092 + 8) >> 4 = 256 -> 255
    assert (4 * 1023 + 8) >> 4 == 256
    assert R.box_plane(p, 10, 1, 1, 1).tolist() == [[255]]


def test_k0_is_the_10_to_8_bit_rule():
    p = np.arange(1024, dtype=np.uint16).reshape(32, 32)
    assert np.array_equal(R.box_plane(p, 10, 0, 32, 32), O.to8(p, 10))
    q = np.arange(256, dtype=np.uint16).reshape(16, 16)
    assert np.array_equal(R.box_plane(q, 8, 0, 16, 16), q.astype(np.uint8))


def test_edges_replicate_the_last_column_and_row():
    p = np.array([[10, 20, 30], [40, 50, 60]], dtype=np.uint16)  # 3 wide, 2 high, s = 2 -> 2 x 1
    out = R.box_plane(p, 8, 1, 2, 1)
    assert out.tolist() == [[(10 + 20 + 40 + 50 + 2) >> 2, (30 + 30 + 60 + 60 + 2) >> 2]]


@pytest.mark.parametrize("w,h,sizes", [
    (72, 40, [(72, 40), (36, 20), (18, 10), (10, 6)]),
    (48, 200, [(48, 200), (24, 100), (12, 50), (6, 26)]),
    (1920, 1080, [(1920, 1080), (960, 540), (480, 270), (240, 136)]),
    (320, 180, [(320, 180), (160, 90), (80, 46), (40, 24)]),
    (64, 64, [(64, 64), (32, 32), (16, 16), (8, 8)]),
])
def test_sizes(w, h, sizes):
    assert [R.scaled_size(w, h, k) for k in range(4)] == sizes


def test_max_dim_rule():
    assert R.resolve_scale(1920, 1080, 0, 512) == 2
    assert R.resolve_scale(1920, 1080, 0, 100) == 3   # none fits: 3
    assert R.resolve_scale(1920, 1080, 0, 4000) == 0
    assert R.resolve_scale(64, 64, 1, 16) == 2        # starts at `scale`
    assert R.resolve_scale(64, 64, 2, 0) == 2         # off


@pytest.mark.parametrize("name,codec", [
    ("hevc/p11_64x64_tiny.h265", 265), ("hevc/p12_72x40_odd_crop.h265", 265),
    ("hevc/p08_320x180_10bit_q2.h265", 265), ("h264/a12_72x40_odd_crop.h264", 264)])
def test_model_at_k0_is_the_oracle_transcode(name, codec):
    s = read(golden(name))
    y8, u8, v8, jpg = R.expected(s, codec, 0)
    assert jpg == O.transcode(s)


def test_model_jpeg_carries_the_scaled_size():
    s = read(golden("hevc/p12_72x40_odd_crop.h265"))
    for k, size in ((1, (36, 20)), (2, (18, 10)), (3, (10, 6))):
        w, h, _, _ = O.jpeg_parse(R.expected(s, 265, k)[3])
        assert (w, h) == size


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


def test_scaled_output_symbols_declared_and_exported():
    host = {"h2j_engine_submit_opts", "h2j_engine_transcode_opts", "h2j_h265_to_jpeg_mem_scaled",
            "h2j_engine_decode_scaled"}
    assert host <= _declared("h2j.h")
    assert host <= _exports("libH265ToJpeg.so")
    assert "h2j_gpu_scale" in _declared("h2j_gpu.h")
    assert "h2j_gpu_scale" in _exports("libh2j_hip.so")
