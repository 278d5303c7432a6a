"""GPU: padded output -- renditions letterboxed to the exact size of their box by K3b (DESIGN.md "Padded output (K3b)").

A padded rendition is its box: the picture part -- the rendition's final 8-bit planes, after orientation, window,
scale / fit and sharpen -- centred in a canvas of the box's size, the rest one colour; the padded planes are the picture
the JPEG or the RGB pixels are made of.  Every expected value is the oracle's decoded planes through the existing models
(orient_ref, crop_ref, scale_ref, resize_ref, finish_ref: test_gpu_rgb's _final_planes), then tests/pad_ref.py, then
finish_ref.encode_q or rgb_ref.convert -- never another call into the engine."""
import ctypes
import functools

import numpy as np
import pytest

import finish_ref as F
import oracle_py as O
import pad_ref as PAD
import rgb_ref as RGB
from test_gpu_rgb import A12, IMG, P01, P08, P11, P12, P15, _final_planes, key, report, same, stream

pytestmark = pytest.mark.gpu

BLACK, GREY, RED = True, (114, 114, 114), (255, 0, 16)  # (RED: Cb and Cr differ from 128 and from each other)

# (stream, the rendition's options without pad, the colour, (picture part, canvas, place))
CASES = [
    (P11, dict(fit=(64, 64)), RED, ((64, 64), (64, 64), (0, 0))),  # no border: the job without pad
    (P11, dict(fit=(70, 66)), GREY, ((64, 64), (70, 66), (2, 0))),  # plain 8-bit; luma shift 2, chroma shift 1; BW % 4 == 2
    (P11, dict(fit=(78, 66)), RED, ((64, 64), (78, 66), (6, 0))),  # chroma shift 3
    (P11, dict(fit=(90, 70)), BLACK, ((64, 64), (90, 70), (12, 2))),  # both axes; chroma shift 2; one fill row above
    (P11, dict(fit=(90, 70), sharpen=16), RED, ((64, 64), (90, 70), (12, 2))),  # a wide source (upic) with both offsets
    (P11, dict(cover=(100, 60)), GREY, ((64, 38), (100, 60), (18, 10))),  # cover of a smaller picture; window at y = 12
    (P12, dict(fit=(50, 50)), RED, ((50, 26), (50, 50), (0, 12))),  # wide (K3r); rows only
    (P15, dict(fit=(16, 16)), RED, ((2, 16), (16, 16), (6, 0))),  # narrower than a dword; the chroma sample at byte 3
    (P15, dict(fit=(46, 100)), GREY, ((24, 100), (46, 100), (10, 0))),  # wide (K3s k = 1); chroma shifts 1, 2, 3
    (P15, dict(fit=(50, 100)), RED, ((24, 100), (50, 100), (12, 0))),
    (P15, dict(fit=(54, 100)), BLACK, ((24, 100), (54, 100), (14, 0))),
    (P01, dict(fit=(6, 6)), RED, ((6, 2), (6, 6), (0, 2))),  # the whole canvas is one partial dword
    (P01, dict(orient=6, fit=(256, 256)), GREY, ((146, 256), (256, 256), (54, 0))),  # an oriented source; chroma at 27
    (P01, dict(crop=(36, 10, 300, 200), fit=(128, 128)), RED, ((128, 84), (128, 128), (0, 22))),  # a windowed source
    (P08, dict(fit=(400, 200)), RED, ((320, 180), (400, 200), (40, 10))),  # plain 16-bit through K4's conversion
    (A12, dict(fit=(80, 48)), GREY, ((72, 40), (80, 48), (4, 4))),  # the other codec's frames
    (IMG, dict(fit=(640, 640)), GREY, ((640, 360), (640, 640), (0, 140))),  # the detector letterbox; a multi-workgroup grid
]


def colour_of(pad):
    return (0, 0, 0) if pad is True else tuple(pad)


@functools.lru_cache(maxsize=None)
def _padded_planes(name, k):
    """The padded planes of the spec (its format and quantiser scale aside), and the picture part's size."""
    spec = dict(k)
    geo = {a: b for a, b in spec.items() if a not in ("qscale", "format", "pad")}
    y, u, v = _final_planes(name, key(geo))
    oh, ow = y.shape
    if not spec.get("pad"):
        return (y, u, v), (ow, oh)
    bw, bh, px, py = PAD.place(ow, oh, *(spec.get("fit") or spec["cover"]))
    if (bw, bh) == (ow, oh):
        return (y, u, v), (ow, oh)
    return PAD.pad_planes(y, u, v, bw, bh, px, py, PAD.pad_colour(colour_of(spec["pad"]))), (ow, oh)


@functools.lru_cache(maxsize=None)
def _expected(name, k):
    spec = dict(k)
    planes, _ = _padded_planes(name, k)
    fmt = spec.get("format") or "jpeg"
    if fmt == "jpeg":
        return F.encode_q(*planes, spec.get("qscale", 0) or 0)
    out = RGB.convert(*planes, fmt)
    out.setflags(write=False)
    return out


def expected(name, spec):
    return _expected(name, key(spec))


def padded_planes(name, spec):
    return _padded_planes(name, key(spec))[0]


def canvas_bytes(bw, bh):
    stride = lambda w: (w + 15) & ~15
    return stride(bw) * bh + 2 * stride(bw // 2) * (bh // 2)


def check(items, outs):
    bad = [(n, sp, report(got, expected(n, sp))) for (n, specs), o in zip(items, outs) for sp, got in zip(specs, o)
           if not same(got, expected(n, sp))]
    assert not bad, bad[:6]


# 1. every case in one batch: as JPEG, rgb and rgb_planar, beside the unpadded rendition of the same geometry and plain items
def test_one_batch_byte_exact(engine):
    items = [(n, [dict(sp, pad=c), dict(sp, pad=c, format="rgb"), sp, dict(sp, pad=c, format="rgb_planar")]) for n, sp, c, _ in CASES]
    items += [(P11, [{}]), (P12, [{}, dict(scale=1)])]
    outs = engine.transcode_multi([stream(n) for n, _ in items], [[s or 0 for s in specs] for _, specs in items])
    assert all(st == 0 for row in engine.last_status for st in row), engine.last_status
    check(items, outs)
    for (n, sp, c, (pic, box, _)), o in zip(CASES, outs):
        assert O.jpeg_parse(o[0])[:2] == box and o[1].shape == (box[1], box[0], 3) and o[3].shape == (3, box[1], box[0]), (n, sp)
        assert O.jpeg_parse(o[2])[:2] == pic
    # no border: the bytes of the call without pad
    assert outs[0][0] == outs[0][2] == expected(P11, dict(fit=(64, 64)))
    # the plain entries are what today's calls return
    assert outs[-2] == [O.transcode(stream(P11))] and outs[-1][0] == O.transcode(stream(P12))
    st = engine.stats()
    assert st["renditions"] == sum(len(specs) for _, specs in items) and st["frames"] == len(items)
    # one canvas an item: the JPEG and the two raw renditions of a letterbox share it; none where nothing is padded
    assert st["pad_bytes"] == sum(canvas_bytes(*box) for _, _, _, (pic, box, _) in CASES if pic != box)
    assert st["raw_bytes"] == sum(2 * 3 * box[0] * box[1] for _, _, _, (_, box, _) in CASES)


# 2. the padded planes themselves, and the placements the rule gives
@pytest.mark.parametrize("case", range(len(CASES)))
def test_planes(engine, case):
    n, sp, c, (pic, box, at) = CASES[case]
    spec = dict(sp, pad=c)
    r = engine.decode_multi7(stream(n), [spec], 0)
    y, u, v = r[:3]
    assert r[3] == box and r[10] == (1 if pic != box else 0) and r[11] == at + pic, (r[3], r[10], r[11])
    if pic != box:
        assert r[12] == PAD.pad_colour(colour_of(c))
    for got, exp in zip((y, u, v), padded_planes(n, spec)):
        assert got.shape == exp.shape and np.array_equal(got, exp), (n, sp, np.argwhere(got != exp)[:4].tolist())


def test_planes_of_the_largest_canvases(engine):
    # H2J_PAD_MAX_SAMPLES: 8192 x 8192 and the widest canvas of as many samples, 65534 x 1024 -- the largest plane offsets
    # and pitches and the widest grid K3b gets; one sample more on either side is refused (tests/test_pad_api.py)
    for fit, c, at in (((8192, 8192), GREY, (4064, 4064)), ((65535, 1025), RED, (32734, 480))):
        spec = dict(fit=fit, pad=c)
        y, u, v, size, _, _, _, _, _, _, padded, place, fill = engine.decode_multi7(stream(P11), [spec], 0)
        assert size == (fit[0] & ~1, fit[1] & ~1) and padded == 1 and place == at + (64, 64) and fill == PAD.pad_colour(c)
        for got, exp in zip((y, u, v), padded_planes(P11, spec)):
            assert got.shape == exp.shape and np.array_equal(got, exp), (fit, np.argwhere(got != exp)[:4].tolist())
    outs = engine.transcode_multi([stream(P11)], [[dict(fit=(8194, 8192), pad=True), dict(fit=(90, 70), pad=True)]])
    assert engine.last_status == [[-60, 0]] and outs[0][1] == expected(P11, dict(fit=(90, 70), pad=True))
    assert "of at most 67108864 samples" in engine.frame_error(0)


# 3. a case alone, a format alone: the launch of one class with one record
@pytest.mark.parametrize("case", [1, 4, 7, 11, 12, 14])
def test_single_rendition(engine, case):
    n, sp, c, (_, box, _) = CASES[case]
    for fmt in ("jpeg", "rgb", "rgb_planar"):
        spec = dict(sp, pad=c, format=fmt)
        got = engine.transcode_multi([stream(n)], [spec])[0][0]
        assert same(got, expected(n, spec)), (n, spec, report(got, expected(n, spec)))
        assert engine.stats()["pad_bytes"] == canvas_bytes(*box)


def test_no_border_launches_nothing(engine):
    got = engine.transcode_multi([stream(P11)], [[dict(fit=(64, 64), pad=RED), dict(fit=(65, 65), pad=GREY, format="rgb")]])[0]
    assert got[0] == O.transcode(stream(P11)) and same(got[1], expected(P11, dict(format="rgb")))
    assert engine.stats()["pad_bytes"] == 0


def test_qscale_and_shared_picture_part(engine):
    # one picture part (K3r 50 x 26, sharpened) under two canvases and an unpadded rendition; a forced scale on a canvas
    rend = [dict(fit=(50, 50), sharpen=8, pad=GREY, qscale=5), dict(fit=(50, 50), sharpen=8), dict(fit=(50, 50), sharpen=8, pad=RED),
            dict(fit=(50, 50), sharpen=8, pad=GREY, format="rgb"), dict(fit=(50, 50), sharpen=8, pad=GREY)]
    outs = engine.transcode_multi([stream(P12)], [rend])
    assert engine.last_status == [[0] * 5]
    check([(P12, rend)], outs)
    assert outs[0][0] != outs[0][4]
    # three canvases: grey at scale 5, red, grey at the rate control's scale (the raw rendition reads the first grey one)
    assert engine.stats()["pad_bytes"] == 3 * canvas_bytes(50, 50)


def test_picture_part_written_by_the_pyramid(engine):
    # 416 x 240 in (208, 130) is 208 x 120, K3s level 1: with levels 2 and 3 beside it K3p writes the picture part, which
    # no JPEG rendition shows; an oriented, sharpened cover in a larger box beside them
    rend = [dict(fit=(208, 130), pad=GREY), dict(scale=2), dict(scale=3), dict(fit=(208, 130), pad=GREY, format="rgb"),
            dict(orient=8, cover=(300, 500), sharpen=24, pad=RED), dict(orient=8, cover=(300, 500), sharpen=24)]
    outs = engine.transcode_multi([stream(P01)], [rend])
    assert engine.last_status == [[0] * 6]
    check([(P01, rend)], outs)
    assert O.jpeg_parse(outs[0][0])[:2] == (208, 130) and O.jpeg_parse(outs[0][4])[:2] == (300, 500)
    assert O.jpeg_parse(outs[0][5])[:2] == (240, 400)  # (nothing upscales: the cover of the 240 x 416 oriented picture)
    assert engine.stats()["pad_bytes"] == canvas_bytes(208, 130) + canvas_bytes(300, 500)


# ---- the C calls through ctypes

def o7(**kw):
    import h2j
    o = h2j.OutOpts7()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def call7(engine, streams, per_item, cap):
    """(rc, status, offs, lens, wh, out) of one multi7 call with the items' option structs."""
    import h2j
    n, flat = len(streams), [o for item in per_item for o in item]
    total = len(flat)
    bufs = [(ctypes.c_uint8 * len(s)).from_buffer_copy(s) for s in streams]
    ptrs = (ctypes.POINTER(ctypes.c_uint8) * n)(*[ctypes.cast(b, ctypes.POINTER(ctypes.c_uint8)) for b in bufs])
    sizes = (ctypes.c_size_t * n)(*[len(s) for s in streams])
    nrend = (ctypes.c_int32 * n)(*[len(item) for item in per_item])
    opts = (h2j.OutOpts7 * total)(*flat)
    out = (ctypes.c_uint8 * cap)()
    offs, lens, status = (ctypes.c_size_t * total)(), (ctypes.c_size_t * total)(), (ctypes.c_int * total)()
    wh = (ctypes.c_int32 * (2 * total))(*([-7] * (2 * total)))
    rc = engine._lib.h2j_engine_transcode_multi7(engine._h, n, ptrs, sizes, nrend, opts, out, cap, offs, lens, status, wh)
    return rc, list(status), list(offs), list(lens), list(wh), bytes(out)


def piece(res, i):
    return res[5][res[2][i]:res[2][i] + res[3][i]]


# 4. a padded raw rendition that does not fit: -50 with the canvas reported, and the Python retry sized from it
def test_too_small_buffer_reports_the_canvas(engine):
    res = call7(engine, [stream(P11), stream(P15)],
                [[o7(fit_w=90, fit_h=70, pad=1, format=1)], [o7(fit_w=16, fit_h=16, pad=1, background=0xFF0010, format=2)]], 1024)
    # 90 x 70 x 3 does not fit 1024 bytes; 16 x 16 x 3 = 768 does
    assert res[0] == -3 and res[1] == [-50, 0], res[:2]
    assert res[4] == [90, 70, 16, 16] and res[3] == [0, 768]
    assert piece(res, 1) == expected(P15, dict(fit=(16, 16), pad=RED, format="rgb_planar")).tobytes()
    assert engine.frame_error(0) == "output buffer too small"
    rend = [[dict(fit=(90, 70), pad=True, format="rgb")], [dict(fit=(16, 16), pad=RED, format="rgb_planar"), dict(fit=(16, 16), pad=RED)]]
    outs = engine.transcode_multi([stream(P11), stream(P15)], rend, out_cap=1024)
    assert engine.last_status == [[0], [0, 0]]
    check(list(zip((P11, P15), rend)), outs)


# 5. the asynchronous form, the keyword forms and the facade agree with the dict form
def test_async_and_keywords_agree(engine):
    rend = [dict(fit=(90, 70), pad=GREY, format="rgb"), dict(fit=(90, 70), pad=GREY), dict(cover=(100, 60), pad=True)]
    res = engine.transcode_multi_async([[stream(P11), stream(P12)], [stream(A12)]], rend)
    assert engine.last_status == [[[0, 0, 0], [0, 0, 0]], [[0, 0, 0]]]
    for names, out in zip(([P11, P12], [A12]), res):
        check([(n, rend) for n in names], out)
    names = [P01, P11]
    got = engine.transcode([stream(n) for n in names], fit=(90, 70), pad=GREY, format="rgb")
    assert engine.last_status == [0, 0]
    for n, g in zip(names, got):
        assert same(g, expected(n, dict(fit=(90, 70), pad=GREY, format="rgb"))), n
    mixed = engine.transcode([stream(n) for n in names], cover=(100, 60), pad=[True, None])
    assert mixed[0] == expected(P01, dict(cover=(100, 60), pad=True)) and mixed[1] == expected(P11, dict(cover=(100, 60)))
    kw = engine.transcode_async([[stream(P12)], [stream(P11)]], fit=(50, 50), pad=[RED, [GREY]], sharpen=16)
    assert kw[0][0] == expected(P12, dict(fit=(50, 50), pad=RED, sharpen=16)) and kw[1][0] == expected(P11, dict(fit=(50, 50), pad=GREY, sharpen=16))


def test_mem_multi7(engine):
    lib = engine._lib
    s = stream(P11)
    buf = (ctypes.c_uint8 * len(s)).from_buffer_copy(s)
    opts = (type(o7()) * 3)(o7(fit_w=70, fit_h=66, pad=1, background=0x727272, format=1), o7(fit_w=70, fit_h=66, pad=1, background=0x727272), o7(pad=1))
    ptr = (ctypes.POINTER(ctypes.c_uint8) * 3)()
    lens, status, wh = (ctypes.c_size_t * 3)(), (ctypes.c_int * 3)(), (ctypes.c_int32 * 6)()
    assert lib.h2j_h265_to_jpeg_mem_multi7(buf, len(s), 3, opts, ptr, lens, status, wh) == 0
    assert list(status) == [0, 0, -60] and list(wh) == [70, 66, 70, 66, 0, 0] and not ptr[2]
    got = [ctypes.string_at(ptr[r], lens[r]) for r in range(2)]
    for r in range(2):
        lib.h2j_free(ptr[r])
    assert got[0] == expected(P11, dict(fit=(70, 66), pad=GREY, format="rgb")).tobytes() and got[1] == expected(P11, dict(fit=(70, 66), pad=GREY))


# 6. invalid options fail alone beside valid renditions of the same item
def test_invalid_options_fail_alone(engine):
    import h2j
    E = h2j.ERR_OUT_OPTS
    res = call7(engine, [stream(P11)],
                [[o7(), o7(fit_w=90, fit_h=70, pad=2), o7(fit_w=90, fit_h=70, pad=1, background=1 << 24), o7(fit_w=90, fit_h=70, background=5),
                  o7(pad=1), o7(fit_w=90, pad=1), o7(fit_w=90, fit_h=70, pad=1, background=0x727272)]], 4 << 20)
    assert res[0] == 0 and res[1] == [0, E, E, E, E, E, 0], res[:2]
    assert piece(res, 0) == O.transcode(stream(P11)) and piece(res, 6) == expected(P11, dict(fit=(90, 70), pad=GREY))
    assert res[4] == [64, 64] + [0, 0] * 5 + [90, 70]
    assert "pad 2 (0..1; needs a box" in engine.frame_error(1) and "background 16777216" in engine.frame_error(2)
    assert "pad 0" in engine.frame_error(3) and "background 5" in engine.frame_error(3) and "pad 1" in engine.frame_error(4)
    assert engine.frame_error(0) == "" and engine.frame_error(6) == ""
    r7 = o7(fit_w=90, fit_h=70, pad=1)
    r7.reserved[0] = 1
    assert call7(engine, [stream(P11)], [[r7, o7()]], 1 << 20)[1] == [E, 0]
    # the words through an opts6 call: the multi6 calls keep rejecting them
    from test_gpu_rgb import call6
    bad6 = h2j.OutOpts6(fit_w=90, fit_h=70)
    bad6.reserved[0] = 1
    res = call6(engine, [stream(P11)], [[h2j.OutOpts6(), bad6]], 1 << 20)
    assert res[0] == 0 and res[1] == [0, E]
    # the Python forms: last_status carries the failures, the entries are None
    outs = engine.transcode_multi([stream(P11)], [[{"pad": True}, {"fit": (90, 70), "pad": True}, 1]])
    assert engine.last_status == [[E, 0, 0]] and outs[0][0] is None and outs[0][1] == expected(P11, dict(fit=(90, 70), pad=True))


# 7. the input-pipeline call: one shape whatever the pictures' sizes
def test_batch_shape(engine):
    names = [P01, P11, P15, P08]
    streams = [stream(n) for n in names]
    ragged = engine.transcode(streams, fit=(224, 224), format="rgb_planar")
    assert len({a.shape for a in ragged}) == 4
    got = engine.transcode(streams, fit=(224, 224), pad=True, format="rgb_planar")
    assert engine.last_status == [0] * 4 and [a.shape for a in got] == [(3, 224, 224)] * 4
    batch = np.stack(got)
    assert batch.shape == (4, 3, 224, 224)
    for n, g in zip(names, got):
        exp = expected(n, dict(fit=(224, 224), pad=True, format="rgb_planar"))
        assert same(g, exp), (n, report(g, exp))
