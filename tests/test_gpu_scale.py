"""GPU: scaled JPEG output (K3s box filter + the JPEG stages on the scaled picture) against the
model in tests/scale_ref.py.  Integer arithmetic with one rounding: every plane and every JPEG
is compared byte for byte; k = 0 items must equal the oracle's unscaled transcode."""
import ctypes
import functools
import glob
import os
import threading

import numpy as np
import pytest

import oracle_py as O
import scale_ref as R
from conftest import golden, read

pytestmark = pytest.mark.gpu

# the smallest shapes that reach each path of K3s / K4 on a scaled picture
SMALL = [
    "hevc/p11_64x64_tiny.h265",               # 8x8 output at k = 3: one MCU, one partial workgroup
    "h264/a11_64x64_tiny.h264",
    "hevc/p12_72x40_odd_crop.h265",           # crop not load-aligned; both edges clamp at k = 3 (10x6)
    "h264/a12_72x40_odd_crop.h264",
    "hevc/p15_48x200_wpp_narrow.h265",        # 6x26: the bottom clamp
    "hevc/p09_200x120_noqpd_notskip.h265",    # 26 wide at k = 3: the right clamp
    "hevc/p25_400x240_conf_left64_top16.h265",  # aligned non-zero crop on the fast path
    "hevc/p01_416x240_q22.h265",              # 8-bit with SAO (pic2 is SAO's output)
    "hevc/p19_480x272_tiles2x2_wpp_nolf.h265",  # SAO off
    "hevc/p26_416x240_9bit.h265",
    "hevc/p08_320x180_10bit_q2.h265",         # 46 rows at k = 2
    "hevc/p27_416x240_12bit.h265",
    "h264/a13_320x180_10bit_q0.h264",
    "h264/a29_192x112_14bit_cavlc_pcm.h264",
    "h264/a45_208x128_mono_lossless.h264",
    "h264/a31_336x192_mbaff_cabac_8x8.h264",
    "h264/a37_320x192_paff_cabac_8x8_slices.h264",
]
# many workgroups and the variance path on a real picture
BIG = ["img01.h265", "img01.h264"]
CASES = [(n, k) for n in SMALL for k in (1, 2, 3)] + [(n, k) for n in BIG for k in (1, 3)]


@functools.lru_cache(maxsize=None)
def stream(name):
    return read(golden(name))


@functools.lru_cache(maxsize=None)
def decoded(name):
    return O.decode(stream(name), R.codec_of(name))


@functools.lru_cache(maxsize=None)
def model(name, k):
    """(Y_k, U_k, V_k, JPEG bytes) of the model; k = 0: the oracle's transcode."""
    y, u, v, bd = decoded(name)
    y8, u8, v8 = R.scale_planes(y, u, v, bd, k)
    return y8, u8, v8, (O.transcode(stream(name)) if k == 0 else R.encode(y8, u8, v8))


@pytest.mark.parametrize("name", SMALL + BIG)
def test_scaled_planes_bit_exact(engine, name):
    for k in ((1, 2, 3) if name in SMALL else (1, 3)):
        y, u, v, kk = engine.decode_scaled(stream(name), scale=k)
        assert kk == k
        ey, eu, ev, _ = model(name, k)
        for g, e, pl in ((y, ey, "Y"), (u, eu, "U"), (v, ev, "V")):
            assert g.shape == e.shape, (k, pl, g.shape, e.shape)
            diff = np.argwhere(g != e)
            assert diff.size == 0, f"k={k} {pl}: {len(diff)} mismatches, first at {diff[:5].tolist()}"


def test_scaled_jpegs_one_batch_byte_exact(engine):
    outs = engine.transcode([stream(n) for n, _ in CASES], scale=[k for _, k in CASES])
    bad = [(n, k, engine.frame_error(i)) for i, ((n, k), o) in enumerate(zip(CASES, outs)) if o != model(n, k)[3]]
    assert not bad, bad


def test_one_batch_mixing_scales(engine):
    """Every parity vector with scales cycling 0..3 and img01.h265 once per scale in one batch: the
    K3s frame map, the per-frame arena regions and max_mcu hold with mixed sizes."""
    names = sorted("hevc/" + os.path.basename(p) for p in glob.glob(golden("hevc/*.h265"))) + \
            sorted("h264/" + os.path.basename(p) for p in glob.glob(golden("h264/*.h264")))
    assert len(names) >= 80
    items = [(n, i % 4) for i, n in enumerate(names)]
    for k in range(4):
        items.insert(7 + 19 * k, ("img01.h265", k))
    outs = engine.transcode([stream(n) for n, _ in items], scale=[k for _, k in items])
    bad = [(n, k, engine.frame_error(i)) for i, ((n, k), o) in enumerate(zip(items, outs)) if o != model(n, k)[3]]
    assert not bad, bad


def test_max_dim(engine):
    s264, p11 = stream("img01.h264"), stream("hevc/p11_64x64_tiny.h265")
    outs = engine.transcode([s264, s264, s264, p11], scale=[0, 0, 0, 1], max_dim=[512, 100, 4000, 16])
    assert outs[0] == model("img01.h264", 2)[3]
    assert O.jpeg_parse(outs[0])[:2] == (480, 270)
    assert outs[1] == model("img01.h264", 3)[3]
    assert O.jpeg_parse(outs[1])[:2] == (240, 136)
    assert outs[2] == O.transcode(s264)
    assert O.jpeg_parse(outs[2])[:2] == (1920, 1080)
    assert outs[3] == model("hevc/p11_64x64_tiny.h265", 2)[3]
    assert O.jpeg_parse(outs[3])[:2] == (16, 16)
    assert engine.decode_scaled(p11, scale=1, max_dim=16)[3] == 2


def test_async_batches_with_cycling_scales(engine):
    """Two asynchronous batches of ~300 small pictures submitted before the first wait, then an
    unscaled synchronous call: state carried between slots and chunks."""
    names = SMALL[:10]
    batches, scales = [], []
    for b in range(2):
        items = [(names[(i + 3 * b) % len(names)], (i + b) % 4) for i in range(300 + b)]
        batches.append(items)
        scales.append([k for _, k in items])
    res = engine.transcode_async([[stream(n) for n, _ in items] for items in batches], scale=scales)
    for items, outs in zip(batches, res):
        bad = [(i, n, k) for i, ((n, k), o) in enumerate(zip(items, outs)) if o != model(n, k)[3]]
        assert not bad, bad[:8]
    outs = engine.transcode([stream(n) for n in names])
    assert outs == [model(n, 0)[3] for n in names]


def test_facade_scaled_in_memory_call(engine):
    import h2j
    lib = h2j.load_library()

    def call(name, k):
        s = stream(name)
        buf = (ctypes.c_uint8 * len(s)).from_buffer_copy(s)
        jpeg, n = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_size_t()
        rc = lib.h2j_h265_to_jpeg_mem_scaled(buf, len(s), k, 0, ctypes.byref(jpeg), ctypes.byref(n))
        assert rc == 0, (name, k, rc)
        out = ctypes.string_at(jpeg, n.value)
        lib.h2j_free(jpeg)
        return out

    assert call("hevc/p01_416x240_q22.h265", 2) == model("hevc/p01_416x240_q22.h265", 2)[3]
    got = {}
    jobs = [("hevc/p01_416x240_q22.h265", 1), ("h264/a13_320x180_10bit_q0.h264", 3)]
    ts = [threading.Thread(target=lambda n=n, k=k: got.__setitem__((n, k), call(n, k))) for n, k in jobs]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for n, k in jobs:
        assert got[(n, k)] == model(n, k)[3], (n, k)


def test_invalid_options_fail_alone(engine):
    import h2j
    p11, p12 = "hevc/p11_64x64_tiny.h265", "hevc/p12_72x40_odd_crop.h265"
    items = [(p11, 1, 0), (p11, 4, 0), (p12, 0, 0), (p11, 0, -1), (p12, 2, 0)]
    outs = engine.transcode([stream(n) for n, _, _ in items], scale=[k for _, k, _ in items],
                            max_dim=[m for _, _, m in items])
    for i in (1, 3):
        assert outs[i] is None
        assert engine.last_status[i] == h2j.ERR_OUT_OPTS
        assert engine.frame_error(i)
    for i in (0, 2, 4):
        assert engine.last_status[i] == 0
        assert engine.frame_error(i) == ""
        assert outs[i] == model(items[i][0], items[i][1])[3], i
