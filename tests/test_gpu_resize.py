"""GPU: exact-size JPEG output (K3r area-average resampler + the JPEG stages on the resized picture)
against the model in tests/resize_ref.py.  Integer arithmetic with one rounding: every plane and
every JPEG is compared byte for byte; a fit that K3s can make must give the bytes of that scale, a
fit no smaller than the picture the oracle's unscaled transcode."""
import ctypes
import functools
import glob
import os
import threading

import numpy as np
import pytest

import oracle_py as O
import resize_ref as R
import scale_ref as S
from conftest import golden, read

pytestmark = pytest.mark.gpu

P11 = "hevc/p11_64x64_tiny.h265"
P01 = "hevc/p01_416x240_q22.h265"
# (vector, fit, stretch): the smallest shapes that reach each way K3r can go wrong
SMALL = [
    (P11, (2, 2), False),        # the whole plane in one sample, chroma 1 x 1
    (P11, (62, 62), False),      # ratio just above 1: nearly every footprint is two taps
    (P11, (34, 34), False),
    (P11, (32, 32), False),      # K3s sizes
    (P11, (8, 8), False),
    (P11, (64, 64), False),      # the picture's own size
    (P11, (4000, 0), False),
    ("hevc/p12_72x40_odd_crop.h265", (50, 0), False),   # unaligned first sample
    ("hevc/p12_72x40_odd_crop.h265", (70, 38), False),
    ("h264/a12_72x40_odd_crop.h264", (50, 0), False),
    ("h264/a12_72x40_odd_crop.h264", (70, 38), False),
    ("hevc/p15_48x200_wpp_narrow.h265", (16, 16), False),  # the height binds, 2 columns
    ("hevc/p09_200x120_noqpd_notskip.h265", (26, 0), False),
    ("hevc/p25_400x240_conf_left64_top16.h265", (300, 0), False),  # non-zero crop
    (P01, (200, 238), True),     # the two axes at different ratios, one near 1
    (P01, (414, 60), True),
    ("hevc/p19_480x272_tiles2x2_wpp_nolf.h265", (320, 0), False),  # SAO off: pic2 == pic
] + [(n, f, False) for n in (
    "hevc/p26_416x240_9bit.h265", "hevc/p08_320x180_10bit_q2.h265", "hevc/p27_416x240_12bit.h265",
    "h264/a13_320x180_10bit_q0.h264", "h264/a29_192x112_14bit_cavlc_pcm.h264") for f in ((300, 0), (30, 0))
] + [(n, (100, 100), False) for n in (
    "h264/a45_208x128_mono_lossless.h264", "h264/a31_336x192_mbaff_cabac_8x8.h264",
    "h264/a37_320x192_paff_cabac_8x8_slices.h264")] + [
    # 3840 x 2160 at 10 bits: 2 Sum + D needs more than 32 bits (the smaller pictures above do not)
    ("bench4k/hevc2160_10b_03.h265", (300, 0), False), ("bench4k/hevc2160_10b_03.h265", (1922, 0), False)]
BIG = [(n, f, False) for n in ("img01.h265", "img01.h264")
       for f in ((1280, 720), (512, 512), (100, 100), (16, 16), (960, 540), (480, 270))]
# fits that resolve to a K3s size: the bytes of that scale (img01.h264 is 1920 x 1080; img01.h265 is
# 2560 x 1440, so for it (1280, 720) is the K3s size and (960, 540), (480, 270) are K3r's)
AS_SCALE = {(P11, (32, 32)): 1, (P11, (8, 8)): 3, ("img01.h264", (960, 540)): 1, ("img01.h264", (480, 270)): 2,
            ("img01.h265", (1280, 720)): 1}
# the picture's own size: the oracle's transcode
AS_PLAIN = {(P11, (64, 64)), (P11, (4000, 0))}
SIZES = {("img01.h265", (512, 512)): (512, 288), ("img01.h264", (512, 512)): (512, 288),
         ("img01.h265", (100, 100)): (100, 56), ("img01.h264", (100, 100)): (100, 56),
         ("img01.h265", (1280, 720)): (1280, 720), ("img01.h264", (1280, 720)): (1280, 720),
         ("img01.h265", (16, 16)): (16, 8), ("img01.h264", (16, 16)): (16, 8)}


@functools.lru_cache(maxsize=None)
def stream(name):
    return read(golden(name))


@functools.lru_cache(maxsize=None)
def decoded(name):
    return O.decode(stream(name), S.codec_of(name))


@functools.lru_cache(maxsize=None)
def model(name, fit, stretch=False):
    """(Y_o, U_o, V_o, JPEG bytes, (W_o, H_o)) of the model; the picture's own size: the oracle's transcode."""
    y, u, v, bd = decoded(name)
    ow, oh = R.fit_size(y.shape[1], y.shape[0], fit, stretch)
    y8, u8, v8 = R.resize_planes(y, u, v, bd, ow, oh)
    same = (ow, oh) == (y.shape[1], y.shape[0])
    return y8, u8, v8, (O.transcode(stream(name)) if same else S.encode(y8, u8, v8)), (ow, oh)


@functools.lru_cache(maxsize=None)
def scale_model(name, k):
    """JPEG bytes of the scaled-output model (tests/scale_ref.py); k = 0: the oracle's transcode."""
    y, u, v, bd = decoded(name)
    return O.transcode(stream(name)) if k == 0 else S.encode(*S.scale_planes(y, u, v, bd, k))


def assert_planes(got, exp, what):
    for g, e, pl in zip(got, exp, "YUV"):
        assert g.shape == e.shape, (what, pl, g.shape, e.shape)
        diff = np.argwhere(g != e)
        assert diff.size == 0, f"{what} {pl}: {len(diff)} mismatches, first at {diff[:5].tolist()}, " \
                               f"got {g[tuple(diff[0])]} expected {e[tuple(diff[0])]}"


@pytest.mark.parametrize("name", sorted({n for n, _, _ in SMALL + BIG}))
def test_resized_planes_bit_exact(engine, name):
    for n, fit, stretch in SMALL + BIG:
        if n != name:
            continue
        y, u, v, size = engine.decode_resized(stream(name), fit, stretch)
        ey, eu, ev, _, esize = model(name, fit, stretch)
        assert size == esize, (fit, stretch, size, esize)
        assert_planes((y, u, v), (ey, eu, ev), f"{name} fit={fit} stretch={stretch}")


def test_resized_jpegs_one_batch_byte_exact(engine):
    cases = SMALL + BIG
    outs = engine.transcode([stream(n) for n, _, _ in cases], fit=[f for _, f, _ in cases],
                            stretch=[s for _, _, s in cases])
    bad = [(n, f, s, engine.frame_error(i)) for i, ((n, f, s), o) in enumerate(zip(cases, outs)) if o != model(n, f, s)[3]]
    assert not bad, bad
    for i, (n, f, s) in enumerate(cases):
        if (n, f) in AS_SCALE:
            assert outs[i] == scale_model(n, AS_SCALE[(n, f)]), (n, f)
        if (n, f) in AS_PLAIN:
            assert outs[i] == O.transcode(stream(n)), (n, f)
        if (n, f) in SIZES:
            assert O.jpeg_parse(outs[i])[:2] == SIZES[(n, f)], (n, f)


def test_fit_equals_scale_and_plain_calls(engine):
    """The same bytes from the fit call, the scale= call and the plain call."""
    s11, img = stream(P11), stream("img01.h264")
    fits = engine.transcode([s11, s11, s11, img, img], fit=[(32, 32), (8, 8), (64, 64), (960, 540), (480, 270)])
    scaled = engine.transcode([s11, s11, s11, img, img], scale=[1, 3, 0, 1, 2])
    assert fits == scaled
    assert fits[2] == engine.transcode([s11])[0] == O.transcode(s11)
    assert engine.transcode([s11], fit=(4000, 0)) == [O.transcode(s11)]


def option_cycle(i, name):
    """Item i of a mixed batch: (scale, fit, stretch) cycling plain, scale=k, fit, stretch."""
    kind = i % 4
    if kind == 0:
        return 0, None, False
    if kind == 1:
        return 1 + (i // 4) % 3, None, False
    fit = (20 + 6 * (i % 37), 18 + 10 * (i % 11))
    return 0, fit, kind == 3


def expected_item(name, scale, fit, stretch):
    return scale_model(name, scale) if fit is None else model(name, fit, stretch)[3]


def test_one_batch_mixing_kinds(engine):
    """Every parity vector with options cycling plain, scale=k, fit, stretch and img01.h265 once per
    mode in one batch: the frame map, the per-frame arena regions and max_mcu hold with mixed kinds."""
    names = sorted("hevc/" + os.path.basename(p) for p in glob.glob(golden("hevc/*.h265"))) + \
            sorted("h264/" + os.path.basename(p) for p in glob.glob(golden("h264/*.h264")))
    assert len(names) >= 80
    items = [(n,) + option_cycle(i, n) for i, n in enumerate(names)]
    for m, opt in enumerate([(0, None, False), (2, None, False), (0, (500, 0), False), (0, (640, 500), True)]):
        items.insert(7 + 19 * m, ("img01.h265",) + opt)
    outs = engine.transcode([stream(n) for n, _, _, _ in items], scale=[k for _, k, _, _ in items],
                            fit=[f for _, _, f, _ in items], stretch=[s for _, _, _, s in items])
    bad = [(n, k, f, s, engine.frame_error(i)) for i, ((n, k, f, s), o) in enumerate(zip(items, outs))
           if o != expected_item(n, k, f, s)]
    assert not bad, bad


def test_async_batches_with_cycling_options(engine):
    """Two asynchronous batches of ~300 small pictures submitted before the first wait, then a
    plain synchronous call: state carried between slots and chunks."""
    names = sorted({n for n, _, _ in SMALL})[:10]
    batches = []
    for b in range(2):
        batches.append([(names[(i + 3 * b) % len(names)],) + option_cycle(i + b, None) for i in range(300 + b)])
    res = engine.transcode_async([[stream(n) for n, _, _, _ in items] for items in batches],
                                 scale=[[k for _, k, _, _ in items] for items in batches],
                                 fit=[[f for _, _, f, _ in items] for items in batches],
                                 stretch=[[s for _, _, _, s in items] for items in batches])
    for items, outs in zip(batches, res):
        bad = [(i, n, k, f, s) for i, ((n, k, f, s), o) in enumerate(zip(items, outs)) if o != expected_item(n, k, f, s)]
        assert not bad, bad[:8]
    outs = engine.transcode([stream(n) for n in names])
    assert outs == [O.transcode(stream(n)) for n in names]


def test_facade_fit_in_memory_call(engine):
    import h2j
    lib = h2j.load_library()

    def call(name, fit, stretch):
        s = stream(name)
        buf = (ctypes.c_uint8 * len(s)).from_buffer_copy(s)
        jpeg, n = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_size_t()
        rc = lib.h2j_h265_to_jpeg_mem_fit(buf, len(s), fit[0], fit[1], h2j.FIT_STRETCH if stretch else 0,
                                          ctypes.byref(jpeg), ctypes.byref(n))
        assert rc == 0, (name, fit, rc)
        out = ctypes.string_at(jpeg, n.value)
        lib.h2j_free(jpeg)
        return out

    assert call(P01, (300, 0), False) == model(P01, (300, 0))[3]
    got = {}
    jobs = [(P01, (200, 238), True), ("h264/a13_320x180_10bit_q0.h264", (30, 0), False), (P11, (34, 34), False)]
    ts = [threading.Thread(target=lambda j=j: got.__setitem__(j, call(*j))) for j in jobs]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for j in jobs:
        assert got[j] == model(*j)[3], j


def test_invalid_options_fail_alone(engine):
    import h2j
    p12 = "hevc/p12_72x40_odd_crop.h265"
    # (vector, scale, fit, stretch): 1, 3, 5, 7 are invalid
    items = [(P11, 0, (34, 34), False), (P11, 0, (1, 0), False), (p12, 0, (50, 0), False), (P11, 0, (34, -2), False),
             (p12, 1, None, False), (P11, 1, (34, 34), False), (P11, 0, (62, 62), False), (P11, 0, None, True)]
    outs = engine.transcode([stream(n) for n, _, _, _ in items], scale=[k for _, k, _, _ in items],
                            fit=[f for _, _, f, _ in items], stretch=[s for _, _, _, s in items])
    for i, (n, k, f, s) in enumerate(items):
        if i in (1, 3, 5, 7):
            assert outs[i] is None, i
            assert engine.last_status[i] == h2j.ERR_OUT_OPTS, i
            assert engine.frame_error(i), i
        else:
            assert engine.last_status[i] == 0, i
            assert engine.frame_error(i) == "", i
            assert outs[i] == expected_item(n, k, f, s), i


def test_nonzero_reserved_fails_alone(engine):
    """h2j_out_opts2.reserved must be 0 (through ctypes: h2j.py never sets it)."""
    import h2j
    lib = h2j.load_library()
    n = 3
    ss = [stream(P11)] * n
    opts = (h2j.OutOpts2 * n)(h2j.OutOpts2(0, 0, 34, 34, 0), h2j.OutOpts2(0, 0, 34, 34, 0), h2j.OutOpts2(0, 0, 0, 0, 0))
    opts[1].reserved[2] = 5
    bufs = [(ctypes.c_uint8 * len(s)).from_buffer_copy(s) for s in ss]
    ptrs = (ctypes.POINTER(ctypes.c_uint8) * n)(*[ctypes.cast(b, ctypes.POINTER(ctypes.c_uint8)) for b in bufs])
    sizes = (ctypes.c_size_t * n)(*[len(s) for s in ss])
    cap = n << 20
    out = (ctypes.c_uint8 * cap)()
    offs, lens, status = (ctypes.c_size_t * n)(), (ctypes.c_size_t * n)(), (ctypes.c_int * n)()
    lib.h2j_engine_transcode_opts2(engine._h, n, ptrs, sizes, opts, out, cap, offs, lens, status)
    assert list(status) == [0, h2j.ERR_OUT_OPTS, 0]
    assert engine.frame_error(1) and engine.frame_error(0) == ""
    mv = memoryview(out)
    assert bytes(mv[offs[0]:offs[0] + lens[0]]) == model(P11, (34, 34))[3]
    assert lens[1] == 0
    assert bytes(mv[offs[2]:offs[2] + lens[2]]) == O.transcode(stream(P11))
