"""GPU: RGB output -- renditions as raw pixels, converted by K3c (DESIGN.md "RGB output (K3c)").

A raw rendition returns the rendition's final 8-bit planes -- after orientation, window, scale / fit and sharpen -- as
8-bit RGB.  Every expected value is the oracle's decoded planes through the existing models (orient_ref, crop_ref,
scale_ref, resize_ref, finish_ref) and then tests/rgb_ref.py -- never another call into the engine."""
import ctypes
import functools

import numpy as np
import pytest

import crop_ref as C
import finish_ref as F
import oracle_py as O
import orient_ref as OR
import resize_ref as R
import rgb_ref as RGB
import scale_ref as S
from conftest import golden, read

pytestmark = pytest.mark.gpu

P01 = "hevc/p01_416x240_q22.h265"
P11 = "hevc/p11_64x64_tiny.h265"
P12 = "hevc/p12_72x40_odd_crop.h265"  # chroma pitch 36
A12 = "h264/a12_72x40_odd_crop.h264"
P15 = "hevc/p15_48x200_wpp_narrow.h265"  # narrower than one lane row
P08 = "hevc/p08_320x180_10bit_q2.h265"
A13 = "h264/a13_320x180_10bit_q0.h264"
IMG = "img01.h264"  # 1920 x 1080

# (stream, the rendition's geometry and finishing): each is checked as "rgb" and as "rgb_planar"
CASES = [
    (P11, {}),
    (P12, {}),
    (P12, dict(scale=2)),  # 18 x 10: W % 4 == 2, the last lane of a row is partial
    (P15, {}),
    (P01, dict(scale=3)),  # 52 x 30
    (P01, dict(fit=(100, 0))),  # K3r
    (P01, dict(fit=(6, 4), stretch=True)),
    (P01, dict(fit=(2, 2), stretch=True)),  # every clamp hits the one chroma sample
    (P01, dict(crop=(36, 10, 300, 200))),  # an unaligned mode-0 window
    (P01, dict(orient=6, cover=(64, 64))),
    (P01, dict(orient=6)),  # an unscaled oriented source
    (P01, dict(sharpen=16, scale=2)),  # reads upic
    (P08, {}),  # 16-bit sources
    (A13, {}),
    (A12, {}),
    # 18 x 128, W % 4 == 2: 3 W H = 27 x 256 bytes, so the two layouts' outputs (and whatever follows them) lie back to
    # back in the chunk's RGB region with no padding between: a store past an output's end lands in its neighbour
    (P15, dict(fit=(18, 128), stretch=True)),
]
FMTS = ("rgb", "rgb_planar")


@functools.lru_cache(maxsize=None)
def stream(name):
    return read(golden(name))


@functools.lru_cache(maxsize=None)
def decoded(name):
    return O.decode(stream(name), S.codec_of(name))


def key(spec):
    if isinstance(spec, tuple):  # a (w, h) pair is a fit
        spec = dict(fit=spec)
    return spec if isinstance(spec, int) else tuple(sorted(spec.items()))


@functools.lru_cache(maxsize=None)
def _final_planes(name, k):
    """The rendition's final 8-bit planes: the spec without its format and quantiser scale, through the models."""
    spec = k if isinstance(k, int) else {a: b for a, b in k if a not in ("qscale", "sharpen", "format")}
    a = 0 if isinstance(k, int) else dict(k).get("sharpen", 0)
    y, u, v, bd = decoded(name)
    r = OR.resolve(y.shape[1], y.shape[0], **OR.spec_fields(spec))
    assert r is not None, (name, k)
    win, (ow, oh), mode, o = r
    wy, wu, wv = C.window_planes(*OR.orient_planes(y, u, v, o), win)
    planes = R.resize_planes(wy, wu, wv, bd, ow, oh) if mode == C.RESAMPLE else S.scale_planes(wy, wu, wv, bd, mode)
    assert planes[0].shape == (oh, ow)
    return F.sharpen_planes(*planes, a)


@functools.lru_cache(maxsize=None)
def _expected(name, k):
    spec = {} if isinstance(k, int) else dict(k)
    planes = _final_planes(name, k)
    fmt = spec.get("format") or "jpeg"
    if fmt == "jpeg":
        return F.encode_q(*planes, spec.get("qscale", 0) or 0)
    out = RGB.convert(*planes, fmt)
    out.setflags(write=False)
    return out


def expected(name, spec):
    return _expected(name, key(spec))


def same(got, exp):
    if isinstance(exp, bytes):
        return isinstance(got, bytes) and got == exp
    return (isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == exp.shape and np.array_equal(got, exp))


def report(got, exp):
    if isinstance(exp, bytes) or not isinstance(got, np.ndarray) or got.shape != exp.shape:
        return f"{type(got).__name__} {getattr(got, 'shape', None) or (got is not None and len(got))} for {getattr(exp, 'shape', None) or len(exp)}"
    d = np.argwhere(got != exp)
    return f"{len(d)} of {exp.size} bytes differ, first at {d[:4].tolist()}: got {got[tuple(d[0])]} expected {exp[tuple(d[0])]}"


def raw(spec, fmt):
    return dict(spec, format=fmt)


# 1. every case in one batch, both layouts, with JPEG renditions of the same geometry and plain JPEG items among them
def test_one_batch_byte_exact(engine):
    items = [(n, [raw(sp, "rgb"), sp or 0, raw(sp, "rgb_planar")]) for n, sp in CASES]
    items += [(P11, [0]), (A13, [0, 1]), (P01, [0, {"scale": 3}, {"scale": 3, "format": "rgb"}, {"scale": 1, "format": "rgb_planar"}])]
    outs = engine.transcode_multi([stream(n) for n, _ in items], [specs for _, specs in items])
    assert all(st == 0 for row in engine.last_status for st in row), engine.last_status
    bad = [(n, sp, report(got, expected(n, sp))) for (n, specs), o in zip(items, outs) for sp, got in zip(specs, o)
           if not same(got, expected(n, sp))]
    assert not bad, bad[:6]
    # shapes: (H, W, 3) and (3, H, W) of the output size
    assert outs[2][0].shape == (10, 18, 3) and outs[2][2].shape == (3, 10, 18) and outs[7][0].shape == (2, 2, 3)
    assert outs[10][0].shape == (416, 240, 3) and outs[9][2].shape == (3, 64, 64)
    # the JPEG entries are the files the calls without a format return
    assert outs[-3] == [O.transcode(stream(P11))] and outs[-1][0] == O.transcode(stream(P01)) and outs[-2][0] == O.transcode(stream(A13))
    assert O.jpeg_parse(outs[4][1])[:2] == (52, 30)
    st = engine.stats()
    nraw = sum(1 for _, specs in items for sp in specs if isinstance(sp, dict) and sp.get("format"))
    assert st["renditions"] == sum(len(specs) for _, specs in items) and st["frames"] == len(items)
    assert st["raw_bytes"] == sum(o.size for row in outs for o in row if isinstance(o, np.ndarray)) and nraw == 2 * len(CASES) + 2


# 2. a case alone, a layout alone: the launch of one class with one record
@pytest.mark.parametrize("case", [0, 2, 8, 11, 12])
def test_single_rendition(engine, case):
    name, sp = CASES[case]
    for fmt in FMTS:
        got = engine.transcode_multi([stream(name)], [raw(sp, fmt)])[0][0]
        assert same(got, expected(name, raw(sp, fmt))), (name, sp, fmt, report(got, expected(name, raw(sp, fmt))))


# 3. 1920 x 1080 unscaled: the multi-workgroup grid, a 6.2 MB output
def test_1080p_unscaled_interleaved(engine):
    got = engine.transcode_multi([stream(IMG)], [{"format": "rgb"}])[0][0]
    exp = expected(IMG, {"format": "rgb"})
    assert exp.shape == (1080, 1920, 3)
    assert same(got, exp), report(got, exp)
    assert engine.stats()["raw_bytes"] == 1920 * 1080 * 3


# ---- the C calls through ctypes

def call6(engine, streams, per_item, cap, fn="h2j_engine_transcode_multi6"):
    """(rc, status, offs, lens, wh, out) of one multi6 (multi5: no wh) call with the items' option structs."""
    n, flat = len(streams), [o for item in per_item for o in item]
    total = len(flat)
    bufs = [(ctypes.c_uint8 * len(s)).from_buffer_copy(s) for s in streams]
    ptrs = (ctypes.POINTER(ctypes.c_uint8) * n)(*[ctypes.cast(b, ctypes.POINTER(ctypes.c_uint8)) for b in bufs])
    sizes = (ctypes.c_size_t * n)(*[len(s) for s in streams])
    nrend = (ctypes.c_int32 * n)(*[len(item) for item in per_item])
    opts = (type(flat[0]) * total)(*flat)
    out = (ctypes.c_uint8 * cap)()
    offs, lens, status = (ctypes.c_size_t * total)(), (ctypes.c_size_t * total)(), (ctypes.c_int * total)()
    wh = (ctypes.c_int32 * (2 * total))(*([-7] * (2 * total)))
    extra = (wh,) if fn.endswith("6") else ()
    rc = getattr(engine._lib, fn)(engine._h, n, ptrs, sizes, nrend, opts, out, cap, offs, lens, status, *extra)
    return rc, list(status), list(offs), list(lens), list(wh), bytes(out)


def o6(**kw):
    import h2j
    o = h2j.OutOpts6()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def piece(res, i):
    return res[5][res[2][i]:res[2][i] + res[3][i]]


# 4. invalid options fail alone
def test_invalid_options_fail_alone(engine):
    import h2j
    E = h2j.ERR_OUT_OPTS
    res = call6(engine, [stream(P01), stream(P11)],
                [[o6(), o6(format=3), o6(format=1, qscale=5), o6(format=1, scale_log2=3), o6(format=-1), o6(scale_log2=3)], [o6(format=2)]], 4 << 20)
    assert res[0] == 0 and res[1] == [0, E, E, 0, E, 0, 0], res[:2]
    assert piece(res, 0) == O.transcode(stream(P01)) and piece(res, 5) == expected(P01, 3)
    assert piece(res, 3) == expected(P01, dict(scale=3, format="rgb")).tobytes()
    assert piece(res, 6) == expected(P11, dict(format="rgb_planar")).tobytes()
    # out_wh: the size of every rendition whose options resolve, JPEG ones too; 0, 0 where they do not
    assert res[4] == [416, 240, 0, 0, 0, 0, 52, 30, 0, 0, 52, 30, 64, 64]
    assert "format 3 (0 JPEG, 1 RGB, 2 planar RGB; not with qscale)" in engine.frame_error(1)
    assert "qscale 5" in engine.frame_error(2) and engine.frame_error(0) == "" and engine.frame_error(3) == ""
    # "rgb" through an opts5 call's reserved word: the multi5 calls keep rejecting it
    bad5 = h2j.OutOpts5()
    bad5.reserved[0] = h2j.FMT_RGB8
    res = call6(engine, [stream(P11)], [[h2j.OutOpts5(), bad5, h2j.OutOpts5(scale_log2=1)]], 1 << 20, "h2j_engine_transcode_multi5")
    assert res[0] == 0 and res[1] == [0, E, 0]
    assert piece(res, 0) == O.transcode(stream(P11)) and piece(res, 2) == expected(P11, 1)
    # the Python forms: last_status carries the failures, the entries are None
    outs = engine.transcode_multi([stream(P11)], [[{"format": "rgb", "qscale": 5}, {"format": "rgb"}, 1]])
    assert engine.last_status == [[E, 0, 0]] and outs[0][0] is None
    assert same(outs[0][1], expected(P11, {"format": "rgb"})) and outs[0][2] == expected(P11, 1)


# 5. a raw rendition that does not fit: -50 with its size reported, and the Python retry sized from it
def test_too_small_buffer_reports_the_size(engine):
    res = call6(engine, [stream(P11), stream(P12), stream(P01)], [[o6(format=1)], [o6(scale_log2=2, format=2)], [o6()]], 1024)
    # 64 x 64 x 3 does not fit 1024 bytes; 18 x 10 x 3 = 540 does, and the 416 x 240 JPEG behind it does not
    assert len(expected(P01, 0)) > 1024 - 540
    assert res[0] == -3 and res[1] == [-50, 0, -50], res[:2]
    assert res[4] == [64, 64, 18, 10, 416, 240] and res[3] == [0, 540, 0]
    assert piece(res, 1) == expected(P12, dict(scale=2, format="rgb_planar")).tobytes()
    assert engine.frame_error(0) == "output buffer too small"
    outs = engine.transcode_multi([stream(P11), stream(P12)], [[{"format": "rgb"}], [{"scale": 2, "format": "rgb_planar"}, 0]], out_cap=1024)
    assert engine.last_status == [[0], [0, 0]]
    assert same(outs[0][0], expected(P11, {"format": "rgb"})) and same(outs[1][0], expected(P12, dict(scale=2, format="rgb_planar")))
    assert outs[1][1] == expected(P12, 0) == O.transcode(stream(P12))


# 6. the asynchronous form and the facade
def test_async_two_batches(engine):
    rend = [{"scale": 1, "format": "rgb"}, 1, {"format": "rgb_planar"}]
    batches = [[stream(P01), stream(P12)], [stream(A12)]]
    res = engine.transcode_multi_async(batches, rend)
    assert engine.last_status == [[[0, 0, 0], [0, 0, 0]], [[0, 0, 0]]]
    for names, out in zip(([P01, P12], [A12]), res):
        for n, o in zip(names, out):
            for sp, got in zip(rend, o):
                assert same(got, expected(n, sp)), (n, sp, report(got, expected(n, sp)))


def test_async_output_larger_than_the_estimate(engine):
    # the asynchronous path cannot know a picture's size before it is parsed: a 960 x 540 raw rendition (1.55 MB) of a
    # 155 KB stream does not fit what is offered first, and comes back from the resubmission sized from out_wh
    rend = [{"scale": 1, "format": "rgb"}, 1]
    res = engine.transcode_multi_async([[stream(IMG), stream(P11)], [stream(P12)]], rend)
    assert engine.last_status == [[[0, 0], [0, 0]], [[0, 0]]]
    for names, out in zip(([IMG, P11], [P12]), res):
        for n, o in zip(names, out):
            for sp, got in zip(rend, o):
                assert same(got, expected(n, sp)), (n, sp, report(got, expected(n, sp)))
    assert res[0][0][0].shape == (540, 960, 3)
    got = engine.transcode_async([[stream(IMG)]], scale=1, format="rgb_planar")[0][0]
    assert same(got, expected(IMG, dict(scale=1, format="rgb_planar")))


# a view that only raw renditions show gets no JPEG: K4 / K5 run on the others, so the payload the chunk produces and
# copies to the host is that of the JPEG renditions alone
def test_raw_only_view_adds_no_payload(engine):
    s = stream(P01)
    alone = engine.transcode_multi([s, stream(P12)], [[0, dict(scale=1, qscale=5)], [0]])
    st0 = engine.stats()
    mixed = engine.transcode_multi([s, stream(P12)], [[{"fit": (224, 224), "format": "rgb"}, 0, {"scale": 2, "format": "rgb_planar"}, dict(scale=1, qscale=5)],
                                                    [{"format": "rgb"}, 0]])
    st1 = engine.stats()
    assert mixed[0][1] == alone[0][0] == O.transcode(s) and mixed[0][3] == alone[0][1] == expected(P01, dict(scale=1, qscale=5))
    assert mixed[1][1] == alone[1][0]
    assert same(mixed[0][0], expected(P01, {"fit": (224, 224), "format": "rgb"}))
    assert same(mixed[0][2], expected(P01, {"scale": 2, "format": "rgb_planar"})) and same(mixed[1][0], expected(P12, {"format": "rgb"}))
    assert st0["payload_bytes"] > 0 and st1["payload_bytes"] == st0["payload_bytes"]
    raw_bytes = mixed[0][0].size + mixed[0][2].size + mixed[1][0].size
    assert st1["raw_bytes"] == raw_bytes


def test_mem_multi6(engine):
    lib = engine._lib
    s = stream(P12)
    buf = (ctypes.c_uint8 * len(s)).from_buffer_copy(s)
    opts = (type(o6()) * 3)(o6(format=1, scale_log2=2), o6(scale_log2=2), o6(format=3))
    ptr = (ctypes.POINTER(ctypes.c_uint8) * 3)()
    lens, status, wh = (ctypes.c_size_t * 3)(), (ctypes.c_int * 3)(), (ctypes.c_int32 * 6)()
    assert lib.h2j_h265_to_jpeg_mem_multi6(buf, len(s), 3, opts, ptr, lens, status, wh) == 0
    assert list(status) == [0, 0, -60] and list(wh) == [18, 10, 18, 10, 0, 0] and not ptr[2]
    got = [ctypes.string_at(ptr[r], lens[r]) for r in range(2)]
    for r in range(2):
        lib.h2j_free(ptr[r])
    assert got[0] == expected(P12, dict(scale=2, format="rgb")).tobytes() and got[1] == expected(P12, 2)


# 7. the keyword forms agree with the dict form
def test_keywords_agree(engine):
    names = [P01, P11]
    streams = [stream(n) for n in names]
    got = engine.transcode(streams, fit=(224, 224), format="rgb")
    assert engine.last_status == [0, 0]
    via = engine.transcode_multi(streams, [{"fit": (224, 224), "format": "rgb"}])
    assert got[0].shape == (128, 224, 3) and got[1].shape == (64, 64, 3)
    for n, g, v in zip(names, got, via):
        exp = expected(n, {"fit": (224, 224), "format": "rgb"})
        assert same(g, exp) and same(v[0], exp), (n, report(g, exp))
    mixed = engine.transcode(streams, scale=[1, 0], format=["rgb_planar", None])
    assert same(mixed[0], expected(P01, dict(scale=1, format="rgb_planar"))) and mixed[1] == O.transcode(stream(P11))
    kw = engine.transcode_async([[stream(P12)], [stream(P11)]], format=["rgb", "jpeg"], sharpen=16)
    assert same(kw[0][0], expected(P12, dict(sharpen=16, format="rgb"))) and kw[1][0] == expected(P11, dict(sharpen=16))


# 8. every existing-call form returns its previous bytes beside raw renditions, and a raw rendition that shares a JPEG
# rendition's planes (whatever its quantiser scale) equals the model too
def test_existing_forms_unchanged_beside_raw(engine):
    names = [P01, A13, P12]
    plain = [O.transcode(stream(n)) for n in names]
    assert engine.transcode([stream(n) for n in names]) == plain
    rend = [{"scale": 1, "format": "rgb"}, 0, 1, dict(scale=1, qscale=6), (100, 0), dict(orient=6), dict(sharpen=16), {"sharpen": 16, "format": "rgb_planar"}]
    outs = engine.transcode_multi([stream(P01), stream(P12)], rend)
    for n, o in zip((P01, P12), outs):
        bad = [(sp, report(got, expected(n, sp))) for sp, got in zip(rend, o) if not same(got, expected(n, sp))]
        assert not bad, (n, bad)
    assert outs[0][1] == plain[0] and outs[1][1] == plain[2]
    st = engine.stats()
    assert (st["parsed"], st["frames"], st["renditions"]) == (2, 2, 16)
