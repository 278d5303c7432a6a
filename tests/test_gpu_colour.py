"""GPU: colour -- renditions normalised from the source's matrix and range to JFIF's by K3v (DESIGN.md "Colour (K3v)").

A converted rendition is the rendition without `colour` on a picture whose 8-bit planes are the normalised planes.
Every expected value is the oracle's decoded planes through the existing models (orient_ref, crop_ref, scale_ref,
resize_ref: test_gpu_rgb's _final_planes), then tests/colour_ref.py, then finish_ref.sharpen_planes, pad_ref, and
finish_ref.encode_q or rgb_ref.convert -- never another call into the engine."""
import functools
import json
import os

import numpy as np
import pytest

import colour_ref as COL
import crop_ref as C
import finish_ref as F
import heif_mux as M
import heif_ref as HR
import oracle_py as O
import orient_ref as OR
import pad_ref as PAD
import resize_ref as R
import rgb_ref as RGB
import scale_ref as S
from conftest import golden, read
from test_gpu_rgb import A12, IMG, P01, P08, P11, P12, P15, _final_planes, key, report, same, stream

pytestmark = pytest.mark.gpu

NOISE = "entropy/noise_mid_512x256_q4.h265"

B709L, B601L, B2020F, JFIF = ("bt709", "limited"), ("bt601", "limited"), ("bt2020", "full"), ("bt601", "full")
GREY = (114, 114, 114)

# (stream, the rendition's options without colour, the output's size): each runs with (709, limited) and (601, limited),
# as JPEG, rgb and rgb_planar, beside the same spec without colour
CASES = [
    (P11, dict(fit=(64, 64)), (64, 64)),  # plain 8-bit; W % 8 = 0
    (P11, dict(fit=(62, 64)), (62, 62)),  # wide (K3r); W % 8 = 6
    (P11, dict(fit=(60, 64)), (60, 60)),  # W % 8 = 4
    (P11, dict(fit=(58, 64)), (58, 58)),  # W % 8 = 2
    (P15, dict(fit=(16, 16)), (2, 16)),  # narrower than a lane
    (P01, dict(fit=(6, 6)), (6, 2)),  # a single chroma row
    (P12, dict(fit=(50, 50)), (50, 26)),  # wide source, K3r
    (P15, dict(fit=(46, 100)), (24, 100)),  # wide source, K3s
    (P01, dict(crop=(38, 10, 300, 200), scale=0), (300, 200)),  # chroma origin 19
    (P01, dict(orient=6, fit=(256, 256)), (146, 256)),  # an oriented source
    (P08, dict(fit=(400, 200)), (320, 180)),  # 16-bit source (the fit does not enlarge)
    (P08, dict(), (320, 180)),
    (A12, dict(), (72, 40)),  # the other codec's frames
    (IMG, dict(fit=(640, 640), pad=GREY, sharpen=16), (640, 640)),  # the whole chain, several workgroups
    # noise over the whole sample range: the fixtures above are natural pictures, whose chroma never reaches the chroma
    # clips (Cb, Cr below 16 or above 240)
    (NOISE, dict(crop=(0, 60, 72, 40)), (72, 40)),
]
COLOURS = (B709L, B601L)
FMTS = (None, "rgb", "rgb_planar")


def with_colour(spec, colour, fmt=None):
    d = dict(spec)
    if colour is not None:
        d["colour"] = colour
    if fmt:
        d["format"] = fmt
    return d


def finish_chain(planes, spec):
    """Normalised (or plain) unsharpened planes -> the rendition's final planes: sharpen, then the pad border."""
    y, u, v = F.sharpen_planes(*planes, spec.get("sharpen", 0) or 0)
    if spec.get("pad"):
        oh, ow = y.shape
        bw, bh, px, py = PAD.place(ow, oh, *(spec.get("fit") or spec["cover"]))
        if (bw, bh) != (ow, oh):
            pad = (0, 0, 0) if spec["pad"] is True else tuple(spec["pad"])
            y, u, v = PAD.pad_planes(y, u, v, bw, bh, px, py, PAD.pad_colour(pad))
    return y, u, v


@functools.lru_cache(maxsize=None)
def _source_planes(name, k):
    """The planes K3v reads: the spec's geometry alone through the models."""
    geo = {a: b for a, b in dict(k).items() if a not in ("qscale", "sharpen", "format", "pad", "colour")}
    return _final_planes(name, key(geo))


@functools.lru_cache(maxsize=None)
def _planes(name, k):
    spec = dict(k)
    src = _source_planes(name, k)
    col = spec.get("colour")
    if col is not None and tuple(col) != JFIF:
        src = COL.convert(*src, *col)
    return finish_chain(src, spec)


def output_of(planes, spec):
    fmt = spec.get("format") or "jpeg"
    if fmt == "jpeg":
        return F.encode_q(*planes, spec.get("qscale", 0) or 0)
    out = RGB.convert(*planes, fmt)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _expected(name, k):
    return output_of(_planes(name, k), dict(k))


def expected(name, spec):
    if isinstance(spec, int):
        spec = dict(scale=spec) if spec else {}
    return _expected(name, key(spec))


def plane_bytes(w, h):
    stride = lambda n: (n + 15) & ~15  # noqa: E731
    return stride(w) * h + 2 * stride(w // 2) * (h // 2)


def picture_size(name, spec):
    y = _source_planes(name, key(spec))[0]
    return y.shape[1], y.shape[0]


def check(items, outs):
    bad = [(n, sp, report(got, expected(n, sp))) for (n, specs), o in zip(items, outs) for sp, got in zip(specs, o)
           if not same(got, expected(n, sp))]
    assert not bad, bad[:6]


EXTRA = [(P11, dict(fit=(64, 64)), B2020F), (P12, dict(fit=(50, 50)), B2020F)]


def test_the_case_list_makes_every_clip_act():
    """From the model alone: Y low, Y high, and Cb and Cr at both ends."""
    clips = set()
    for n, sp, _ in CASES:
        for col in COLOURS:
            for nm, s, sh in zip("YUV", COL.sums(*_source_planes(n, key(sp)), *col), (20, 16, 16)):
                clips |= ({nm + "lo"} if int(s.min()) < 0 else set()) | ({nm + "hi"} if (int(s.max()) >> sh) > 255 else set())
    assert clips == {"Ylo", "Yhi", "Ulo", "Uhi", "Vlo", "Vhi"}, clips


# 1. every case in one batch, with both colours, as JPEG, rgb and rgb_planar, beside the same spec without colour
def test_one_batch_byte_exact(engine):
    items = [(n, [with_colour(sp, c, f) for c in COLOURS for f in FMTS] + [sp or 0]) for n, sp, _ in CASES]
    items += [(n, [with_colour(sp, c, f) for f in FMTS] + [sp]) for n, sp, c in EXTRA]
    items += [(P11, [with_colour(dict(fit=(64, 64)), JFIF, f) for f in FMTS] + [dict(fit=(64, 64), format=f) if f else dict(fit=(64, 64)) for f in FMTS]),
              (P11, [0]), (P12, [0, dict(scale=1)])]
    outs = engine.transcode_multi([stream(n) for n, _ in items], [specs for _, specs in items])
    assert all(st == 0 for row in engine.last_status for st in row), (engine.last_status, [engine.frame_error(i) for i in range(8)])
    check(items, outs)
    for (n, sp, size), o in zip(CASES, outs):
        assert O.jpeg_parse(o[0])[:2] == size and o[1].shape == (size[1], size[0], 3) and o[5].shape == (3, size[1], size[0]), (n, sp)
        assert o[0] != o[6] and o[3] != o[6] and o[0] != o[3]  # the conversions change the picture, each in its way
    # a source that is JFIF's already: the bytes of the call without colour
    j = outs[len(CASES) + len(EXTRA)]
    assert j[0] == j[3] and np.array_equal(j[1], j[4]) and np.array_equal(j[2], j[5])
    # the plain entries are what today's calls return
    assert outs[-2] == [O.transcode(stream(P11))] and outs[-1][0] == O.transcode(stream(P12))
    st = engine.stats()
    assert st["renditions"] == sum(len(specs) for _, specs in items) and st["frames"] == len(items)
    # one conversion per (geometry, colour): the JPEG and the two raw renditions share it; none for the JFIF source
    want = sum(len(COLOURS) * plane_bytes(*picture_size(n, sp)) for n, sp, _ in CASES) + sum(plane_bytes(*picture_size(n, sp)) for n, sp, _ in EXTRA)
    assert st["colour_bytes"] == want, (st["colour_bytes"], want)


# 2. the planes K4 reads, and what the option resolved to
@pytest.mark.parametrize("case", range(len(CASES)))
def test_planes(engine, case):
    n, sp, size = CASES[case]
    for col in COLOURS:
        spec = with_colour(sp, col)
        r = engine.decode_multi8(stream(n), [spec], 0)
        assert r[3] == size and r[13:] == (COL.MC[col[0]], 1 if col[1] == "full" else 0, 1), (r[3], r[13:])
        for got, exp in zip(r[:3], _planes(n, key(spec))):
            assert got.shape == exp.shape and np.array_equal(got, exp), (n, sp, col, np.argwhere(got != exp)[:4].tolist())
    r = engine.decode_multi8(stream(n), [with_colour(sp, JFIF)], 0)
    assert r[13:] == (6, 1, 0)
    for got, exp in zip(r[:3], _planes(n, key(sp))):
        assert np.array_equal(got, exp)


def test_jfif_source_is_the_call_without_colour(engine):
    sp = dict(fit=(50, 50))
    a = engine.transcode_multi([stream(P12)], [[with_colour(sp, JFIF), with_colour(sp, JFIF, "rgb")]])[0]
    assert engine.stats()["colour_bytes"] == 0
    b = engine.transcode_multi([stream(P12)], [[sp, dict(sp, format="rgb")]])[0]
    assert a[0] == b[0] == expected(P12, sp) and np.array_equal(a[1], b[1])


# 3. auto: the stream's signalling, the file's nclx property over it
def manifest():
    with open(golden("colour/manifest.json")) as f:
        return json.load(f)


def model_of(decoded, spec, sei=0):
    """_final_planes on planes that are no fixture of test_gpu_rgb's: the geometry through the same models."""
    y, u, v, bd = decoded
    geo = {a: b for a, b in spec.items() if a not in ("qscale", "sharpen", "format", "pad", "colour")}
    win, (ow, oh), mode, o = OR.resolve(y.shape[1], y.shape[0], sei=sei, **OR.spec_fields(geo))
    wy, wu, wv = C.window_planes(*OR.orient_planes(y, u, v, o), win)
    return R.resize_planes(wy, wu, wv, bd, ow, oh) if mode == C.RESAMPLE else S.scale_planes(wy, wu, wv, bd, mode)


def expected_auto(decoded, spec, matrix, full):
    src = model_of(decoded, spec)
    col = (COL.MC_NAME[matrix], "full" if full else "limited")
    if col != JFIF:
        src = COL.convert(*src, *col)
    return output_of(finish_chain(src, spec), spec)


def patch_nclx(heic, primaries, transfer, matrix, full):
    import re
    import struct
    out = bytearray(heic)
    at = [m.end() for m in re.finditer(re.escape(b"colrnclx"), heic)]
    assert at
    for a in at:
        out[a:a + 7] = struct.pack(">HHHB", primaries, transfer, matrix, 0x80 if full else 0)
    return bytes(out)


AUTO_SPECS = [dict(colour="auto"), dict(colour="auto", format="rgb"), dict(colour="auto", fit=(30, 30), sharpen=8)]


def test_auto_on_the_vectors(engine):
    ms = manifest()
    streams = [read(golden("colour/" + m["file"])) for m in ms]
    outs = engine.transcode_multi(streams, [AUTO_SPECS + [0] for _ in ms])
    seen = 0
    for m, s, o, st, i in zip(ms, streams, outs, engine.last_status, range(len(ms))):
        dec = O.decode(s, m["codec"])
        if m["matrix"] == 8:  # not converted: the auto renditions fail alone, the value in their message
            assert st == [-60, -60, -60, 0] and o[:3] == [None] * 3, st
            for r in range(3):
                assert "matrix_coefficients 8" in engine.frame_error(4 * i + r), engine.frame_error(4 * i + r)
        else:
            assert st == [0] * 4, (m["file"], st)
            for sp, got in zip(AUTO_SPECS, o):
                exp = expected_auto(dec, sp, m["matrix"], m["full_range"])
                assert same(got, exp), (m["file"], sp, report(got, exp))
            seen += 1
        assert o[3] == S.encode(*S.scale_planes(*dec[:3], dec[3], 0)), m["file"]  # the sibling without colour
    assert seen == len(ms) - 1 == 5
    # the two unscaled auto renditions of a vector share one conversion, the fitted one has its own; the vector whose
    # source is JFIF's (no description, full range) has none
    conv = [(m, s) for m, s in zip(ms, streams) if m["matrix"] != 8 and (COL.MC_NAME[m["matrix"]], m["full_range"]) != ("bt601", 1)]
    assert len(conv) == 4
    assert engine.stats()["colour_bytes"] == sum(plane_bytes(m["w"], m["h"]) + plane_bytes(*model_of(O.decode(s, m["codec"]), AUTO_SPECS[2])[0].shape[::-1])
                                                 for m, s in conv)


def test_auto_on_patched_heics(engine):
    ms = {m["file"]: m for m in manifest()}
    v709 = read(golden("colour/c709_limited.hevc"))   # VUI: BT.709 limited
    novui = read(golden("colour/cnovui.avc"))
    d709, dno = O.decode(v709, 265), O.decode(novui, 264)
    case = next(c for c in HR.CASES if c[0] == "a")
    grid = M.mux(list(HR.tiles(case[0]))[:case[1] * case[2]], grid=(case[2], case[1], case[3], case[4]))
    dgrid = HR.canvas(*case)
    assert ms["c709_limited.hevc"]["matrix"] == 1
    files = [
        (M.mux([v709]), d709, (1, 1)),                                   # the nclx heif_mux writes (709 full) over the VUI (709 limited)
        (patch_nclx(M.mux([v709]), 9, 16, 9, 0), d709, (9, 0)),
        (patch_nclx(M.mux([v709]), 1, 13, 6, 1), d709, (6, 1)),          # JFIF's: nothing to convert
        (patch_nclx(M.mux([v709]), 2, 2, 2, 0), d709, (2, 0)),           # unspecified: BT.601, limited
        (M.mux([v709]).replace(b"colrnclx", b"colrprof"), d709, (1, 0)),  # no nclx: the VUI stands
        (patch_nclx(M.mux([novui], codec=264), 5, 6, 5, 0), dno, (5, 0)),
        (grid, dgrid, (1, 1)),                                           # the grid item has no colr: its tiles'
        (patch_nclx(grid, 9, 16, 9, 0), dgrid, (9, 0)),
    ]
    specs = [dict(colour="auto"), dict(colour="auto", fit=(40, 40), format="rgb_planar"), 0]
    outs = engine.transcode_multi([f for f, _, _ in files], [specs for _ in files])
    assert all(st == [0, 0, 0] for st in engine.last_status), (engine.last_status, engine.frame_error(0))
    for (f, dec, (mc, full)), o in zip(files, outs):
        for sp, got in zip(specs[:2], o):
            exp = expected_auto(dec, sp, mc, full)
            assert same(got, exp), (mc, full, sp, report(got, exp))
        assert o[2] == S.encode(*S.scale_planes(*dec[:3], dec[3], 0))
    # a matrix the library does not convert fails the auto rendition alone
    bad = patch_nclx(M.mux([v709]), 1, 1, 0, 1)
    o = engine.transcode_multi([bad], [[dict(colour="auto"), 0, dict(colour=B709L)]])[0]
    assert engine.last_status[0] == [-60, 0, 0] and o[0] is None and "matrix_coefficients 0" in engine.frame_error(0)
    assert o[2] == expected_auto(d709, dict(colour=B709L), 1, 0)  # an explicit source stands whatever the file says


# 4. sharing, and plain items beside converted ones
def test_sharing_and_mixed_batches(engine):
    sp = dict(fit=(50, 50))
    specs = [with_colour(sp, B709L), with_colour(sp, B709L, "rgb"), with_colour(sp, B709L, "rgb_planar"), dict(sp, colour=B709L, qscale=5),
             dict(sp, colour=B709L, sharpen=16), sp]
    o = engine.transcode_multi([stream(P12)], [specs])[0]
    assert engine.last_status[0] == [0] * 6
    check([(P12, specs)], [o])
    assert engine.stats()["colour_bytes"] == plane_bytes(50, 26)  # five renditions, one conversion
    # mixed colour and plain items in one batch: the plain items' bytes are the oracle's
    names = [P11, P12, A12, P08, P01]
    rends = [[0], [with_colour({}, B709L)], [0, with_colour(dict(scale=1), B601L)], [with_colour({}, B2020F, "rgb")], [0, 1]]
    outs = engine.transcode_multi([stream(n) for n in names], rends)
    assert all(s == 0 for row in engine.last_status for s in row)
    check(list(zip(names, rends)), outs)
    for n, o in zip(names, outs):
        if n in (P11, A12, P01):
            assert o[0] == O.transcode(stream(n)), n
    # the keyword form
    got = engine.transcode([stream(P11), stream(P12)], colour=[B709L, None])
    assert got[0] == expected(P11, dict(colour=B709L)) and got[1] == O.transcode(stream(P12))
