"""GPU: finishing -- a fixed JPEG quantiser scale and the K3u unsharp mask (DESIGN.md "Finishing (K3u, forced
qscale)").

The one definition: the sharpened planes are the picture.  A rendition with `sharpen` returns the bytes the same
call without it returns for a picture whose 8-bit planes are the sharpened planes; `qscale` replaces the rate
control's scale.  Every expected value is the oracle's decoded planes through the existing models (orient_ref,
crop_ref, scale_ref, resize_ref) and then tests/finish_ref.py -- never another call into the engine."""
import functools

import numpy as np
import pytest

import crop_ref as C
import finish_ref as F
import oracle_py as O
import orient_ref as OR
import resize_ref as R
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


def sh(a, **kw):
    return dict(sharpen=a, **kw)


def qs(q, **kw):
    return dict(qscale=q, **kw)


PLANE_CASES = [
    (P11, [sh(1), sh(16), sh(64)]),
    (P12, [sh(1), sh(16), sh(64)]),
    (P15, [sh(16)]),
    (P01, [1, sh(16, scale=2), 3]),  # K3p; sharpen on one level only
    (P01, [1, 2, sh(16, scale=2), qs(5, scale=2)]),  # two more views at a level of the pyramid: K3s writes theirs
    (P01, [sh(16, fit=(100, 0))]),  # K3r
    (P01, [sh(32, fit=(6, 4), stretch=True), sh(64, fit=(2, 2), stretch=True)]),  # 2 x 2: both clamps hit one sample
    (P01, [sh(16, crop=(36, 10, 300, 200), scale=1), sh(16, crop=(36, 10, 300, 200))]),  # the second: an unaligned unscaled window
    (P01, [sh(24, orient=6, cover=(64, 64)), sh(16, orient=6)]),  # the second: an unscaled oriented source
    (P08, [sh(16)]),  # 16-bit unscaled sources
    (A13, [sh(16), sh(40, qscale=7)]),
    (A12, [sh(16)]),
]
QSCALES = [2, 3, 8, 17, 31]


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


def finish_of(spec):
    if isinstance(spec, int):
        return 0, 0
    return spec.get("qscale", 0) or 0, spec.get("sharpen", 0) or 0


@functools.lru_cache(maxsize=None)
def _unfinished(name, k):
    """(window, 8-bit planes, mode, orientation) of the spec without its finishing keys; None: invalid options."""
    spec = k if isinstance(k, int) else {a: b for a, b in k if a not in ("qscale", "sharpen")}
    y, u, v, bd = decoded(name)
    r = OR.resolve(y.shape[1], y.shape[0], **OR.spec_fields(spec))
    if r is None:
        return None
    win, (ow, oh), mode, o = r
    wy, wu, wv = C.window_planes(*OR.orient_planes(y, u, v, o), win)
    planes = R.resize_planes(wy, wu, wv, bd, ow, oh) if mode == C.RESAMPLE else S.scale_planes(wy, wu, wv, bd, mode)
    assert planes[0].shape == (oh, ow)
    return win, planes, mode, o


@functools.lru_cache(maxsize=None)
def _model(name, k):
    """(window, finished 8-bit planes, JPEG bytes, mode, orientation, the qscale K4 uses); None: invalid options."""
    spec = k if isinstance(k, int) else dict(k)
    q, a = finish_of(spec)
    un = _unfinished(name, k)
    if un is None or not (q == 0 or 2 <= q <= 31) or not 0 <= a <= 64:
        return None
    win, planes, mode, o = un
    y8, u8, v8, jpg = F.finish(*planes, qscale=q, sharpen=a)
    return win, (y8, u8, v8), jpg, mode, o, q or O.jpeg_coeffs(y8, u8, v8)[0]


def expected(name, spec):
    m = _model(name, key(spec))
    return None if m is None else m[2]


def assert_planes(got, exp, what):
    for g, e, pl in zip(got, exp, "YUV"):
        assert g.shape == e.shape, (what, pl, g.shape, e.shape)
        diff = np.argwhere(g != e)
        assert diff.size == 0, f"{what} {pl}: {len(diff)} mismatches, first at {diff[:5].tolist()}, " \
                               f"got {g[tuple(diff[0])]} expected {e[tuple(diff[0])]}"


# 1. planes and the scale K4 used, through decode_multi5 with the case's renditions in flight
@pytest.mark.parametrize("case", range(len(PLANE_CASES)))
def test_finished_planes_bit_exact(engine, case):
    name, specs = PLANE_CASES[case]
    for pick, spec in enumerate(specs):
        win, planes, _, mode, o, q = _model(name, key(spec))
        y, u, v, size, m, w, ro, so, gq, ga = engine.decode_multi5(stream(name), specs, pick)
        assert (w, size, ro, so) == (win, (planes[0].shape[1], planes[0].shape[0]), o, 0), (name, spec, w, size, ro)
        assert m in ((5, mode) if mode in (1, 2, 3) else (mode,)), (name, spec, m)
        assert (gq, ga) == (q, finish_of(spec)[1]), (name, spec, gq, ga)
        assert_planes((y, u, v), planes, f"{name} {spec}")


# 2. files: every case in one batch, with plain items among them
def test_finished_jpegs_one_batch_byte_exact(engine):
    items = [(n, list(specs)) for n, specs in PLANE_CASES] + [(P11, [0]), (A13, [0, 1]), (P01, [0])]
    outs = engine.transcode_multi([stream(n) for n, _ in items], [specs for _, specs in items])
    bad = [(n, sp) for (n, specs), o in zip(items, outs) for sp, got in zip(specs, o) if got != expected(n, sp)]
    assert not bad, bad[:8]
    assert all(st == 0 for row in engine.last_status for st in row)
    assert outs[-3] == [O.transcode(stream(P11))] and outs[-1] == [O.transcode(stream(P01))] and outs[-2][0] == O.transcode(stream(A13))
    assert O.jpeg_parse(outs[6][1])[:2] == (2, 2) and O.jpeg_parse(outs[8][0])[:2] == (64, 64)
    # sharpening changed something: the sharpened rendition is not the unsharpened one
    assert outs[3][1] != expected(P01, 2) and outs[4][2] != outs[4][1]


# 3. forced quantiser scales
def test_forced_qscales_byte_exact(engine):
    rend = [qs(q) for q in QSCALES]
    outs = engine.transcode_multi([stream(P12), stream(P01)], rend)
    for name, o in zip((P12, P01), outs):
        assert o == [expected(name, sp) for sp in rend], name
        assert len(o[0]) > len(o[-1])  # a coarser quantiser: fewer bytes
    assert engine.stats()["renditions"] == 10 and engine.stats()["frames"] == 2
    # the DQT of the file is the matrix of the forced scale
    assert sorted(O.jpeg_parse(outs[0][3])[2]) == sorted(int(x) for x in F.matrix(17)[0])


def test_qscale_sweep(engine):
    sweep = [qs(q) for q in range(2, 32)]
    per_item = [sweep[i:i + 8] for i in range(0, len(sweep), 8)]
    outs = engine.transcode_multi([stream(P11)] * len(per_item), per_item)
    got = [j for item in outs for j in item]
    assert got == [expected(P11, sp) for sp in sweep]


def test_forced_qscale_of_the_rate_control_is_the_default(engine):
    for name, spec in ((P01, {}), (P12, dict(scale=1)), (P08, {})):
        q = engine.decode_multi5(stream(name), [dict(spec, sharpen=0)], 0)[8]
        assert 2 <= q <= 31 and q == _model(name, key(dict(spec, sharpen=0)))[5]
        plain, forced = engine.transcode_multi([stream(name)], [spec or 0, dict(spec, qscale=q)])[0]
        assert plain == forced == expected(name, spec or 0) and expected(name, dict(spec, qscale=q)) == plain


def test_rendition_list_from_one_decode(engine):
    rend = [0, qs(2), qs(31), dict(scale=2, qscale=5, sharpen=16)]
    names = [P01, A13]
    outs = engine.transcode_multi([stream(n) for n in names], rend)
    st = engine.stats()
    assert (st["parsed"], st["frames"], st["renditions"]) == (2, 2, 8)
    for n, o in zip(names, outs):
        assert o[0] == O.transcode(stream(n)) and o == [expected(n, sp) for sp in rend], n
        for sp, j in zip(rend, o):  # each equals its single call
            assert engine.transcode_multi([stream(n)], [sp])[0][0] == j, (n, sp)
    # renditions that resolve to the same output, finishing included, are encoded once and hold the same bytes
    outs = engine.transcode_multi([stream(P01)], [sh(16, qscale=4), 0, dict(sharpen=16, qscale=4, scale=0), qs(4)])[0]
    assert outs[0] == outs[2] == expected(P01, sh(16, qscale=4)) and outs[3] == expected(P01, qs(4)) and outs[1] == O.transcode(stream(P01))


def test_finished_1080p(engine):
    spec = dict(scale=1, sharpen=16, qscale=4)
    out = engine.transcode_multi([stream(IMG)], [spec])[0][0]
    assert O.jpeg_parse(out)[:2] == (960, 540)
    assert out == expected(IMG, spec)


# 4. invalid options fail alone
def test_invalid_finishing_fails_alone(engine):
    import h2j
    rend = [0, qs(1), sh(16), qs(32), sh(65), sh(-1), qs(-1), qs(8)]
    for b in (rend[1], rend[3], rend[4], rend[5], rend[6]):
        assert expected(P01, b) is None
    outs = engine.transcode_multi([stream(P01), stream(P11)], [rend, [sh(16)]])
    E = h2j.ERR_OUT_OPTS
    assert engine.last_status == [[0, E, 0, E, E, E, E, 0], [0]]
    assert outs[0] == [expected(P01, sp) for sp in rend] and outs[1] == [expected(P11, sh(16))]
    assert "qscale 1 (0 or 2..31)" in engine.frame_error(1) and "sharpen 65 (0..64)" in engine.frame_error(4)
    assert engine.frame_error(0) == "" and engine.frame_error(2) == ""


# 5. the keyword forms agree with transcode_multi
def test_keywords_agree(engine):
    got = engine.transcode([stream(P01), stream(P11), stream(P12)], qscale=[5, None, 3], sharpen=[16, None, None], scale=[1, 0, 0])
    assert engine.last_status == [0, 0, 0]
    assert got == [expected(P01, dict(scale=1, qscale=5, sharpen=16)), O.transcode(stream(P11)), expected(P12, qs(3))]
    assert engine.transcode([stream(P12)], sharpen=24) == [expected(P12, sh(24))]
    kw = engine.transcode_async([[stream(P01), stream(P11)], [stream(A13)]], qscale=[[8, None], 4], sharpen=16)
    assert kw == [[expected(P01, dict(qscale=8, sharpen=16)), expected(P11, sh(16))], [expected(A13, dict(qscale=4, sharpen=16))]]


# 6. every existing-call form returns its previous bytes in a batch that also holds finishing renditions
def test_existing_forms_unchanged_beside_finishing(engine):
    names = [P01, A13, P12]
    plain = [O.transcode(stream(n)) for n in names]
    assert engine.transcode([stream(n) for n in names]) == plain
    assert engine.transcode([stream(n) for n in names], scale=1) == [expected(n, 1) for n in names]
    assert engine.transcode([stream(P01)], fit=(100, 0)) == [expected(P01, dict(fit=(100, 0)))]
    rend = [0, 1, (100, 0), dict(crop=(36, 10, 300, 200), scale=1), dict(orient=6), sh(16), qs(6, scale=1)]
    rend12 = [0, 1, (50, 0), dict(crop=(4, 2, 40, 30)), dict(orient=6), sh(16), qs(6, scale=1)]
    outs = engine.transcode_multi([stream(P01), stream(P12)], [rend, rend12])
    assert outs[0] == [expected(P01, sp) for sp in rend] and outs[1] == [expected(P12, sp) for sp in rend12]
    assert outs[0][0] == plain[0] and outs[1][0] == plain[2]


def test_finished_output_opens_in_pillow(engine):
    import io
    try:
        from PIL import Image
    except ImportError:  # nothing else rests on Pillow
        return
    out = engine.transcode([stream(P01)], sharpen=16, qscale=4, scale=1)[0]
    im = Image.open(io.BytesIO(out))
    im.load()
    assert im.size == (208, 120)
