"""GPU: oriented output -- renditions rotated and mirrored by K3o (DESIGN.md "Orientation (K3o)").

The one definition: the oriented picture is the picture.  A rendition with an orientation returns the bytes
the same call with its remaining options returns for a picture whose cropped planes are the oriented planes.
So every expected value is the oracle's decoded planes after tests/orient_ref.py's table (numpy slicing and
rot90), through the existing models (crop_ref, scale_ref, resize_ref, scale_ref.encode) -- no new
arithmetic, and never another call into the engine."""
import ctypes
import functools
import threading

import numpy as np
import pytest

import crop_ref as C
import oracle_py as O
import orient_ref as OR
import resize_ref as R
import scale_ref as S
from conftest import golden, read

pytestmark = pytest.mark.gpu

P01 = "hevc/p01_416x240_q22.h265"  # SAO on; 6.5 x 3.75 tiles; oriented width 240 = 15 x 16: the variance-fold predicate holds
P11 = "hevc/p11_64x64_tiny.h265"   # luma one tile exactly, chroma half a tile
P12 = "hevc/p12_72x40_odd_crop.h265"  # chroma pitch 36, edge tiles both ways, unaligned source origins
A12 = "h264/a12_72x40_odd_crop.h264"
P15 = "hevc/p15_48x200_wpp_narrow.h265"  # narrower than a tile, taller than three
P19 = "hevc/p19_480x272_tiles2x2_wpp_nolf.h265"  # pic2 == pic
P25 = "hevc/p25_400x240_conf_left64_top16.h265"  # source origin moved by the conformance crop
P08 = "hevc/p08_320x180_10bit_q2.h265"
P27 = "hevc/p27_416x240_12bit.h265"
A13 = "h264/a13_320x180_10bit_q0.h264"
A31 = "h264/a31_336x192_mbaff_cabac_8x8.h264"
A37 = "h264/a37_320x192_paff_cabac_8x8_slices.h264"
IMG = "img01.h264"  # 1920 x 1080


def ori(o, **kw):
    return dict(orient=o, **kw)


ALL = [ori(o) for o in range(2, 9)]
CASES = [
    (P11, ALL),
    (P12, ALL),
    (A12, ALL),
    (P15, [ori(2), ori(4), ori(5), ori(6), ori(7)]),
    (P25, [ori(3), ori(6), ori(8)]),
    (P01, [ori(2), ori(3), ori(5), ori(6), ori(8)]),
    (P08, [ori(3), ori(5), ori(6)]),
    (P27, [ori(3), ori(5), ori(6)]),
    (A13, [ori(3), ori(5), ori(6)]),
    (A31, [ori(6)]),
    (A37, [ori(6)]),
    (P19, [ori(8)]),
    # composition on p01: the K3p pyramid of an oriented source; a shifted window in oriented coordinates; K3r;
    # cover; the unscaled aligned window of an oriented SAO picture
    (P01, [ori(6, scale=1), ori(6, scale=2), ori(6, scale=3)]),
    (P01, [ori(8, crop=(36, 10, 200, 300), scale=1), ori(5, fit=(100, 0)), ori(6, cover=(64, 64)), ori(3, crop=(16, 16, 208, 112))]),
]


@functools.lru_cache(maxsize=None)
def stream(name):
    return read(golden(name))


@functools.lru_cache(maxsize=None)
def decoded(name):
    return O.decode(stream(name), S.codec_of(name))


def key(spec):
    return spec if isinstance(spec, int) else tuple(sorted(spec.items()))


@functools.lru_cache(maxsize=None)
def _model(name, k, sei=0):
    """(window, 8-bit planes, JPEG bytes, mode, orientation); None: invalid options."""
    spec = k if isinstance(k, int) else dict(k)
    y, u, v, bd = decoded(name)
    r = OR.resolve(y.shape[1], y.shape[0], sei=sei, **OR.spec_fields(spec))
    if r is None:
        return None
    win, (ow, oh), mode, o = r
    oy, ou, ov = OR.orient_planes(y, u, v, o)
    wy, wu, wv = C.window_planes(oy, ou, ov, win)
    if mode == C.RESAMPLE:
        planes = R.resize_planes(wy, wu, wv, bd, ow, oh)
    else:
        planes = S.scale_planes(wy, wu, wv, bd, mode)  # mode 0: the 8-bit conversion alone
    assert planes[0].shape == (oh, ow)
    whole = o == 0 and win == (0, 0, y.shape[1], y.shape[0]) and mode == 0
    return win, planes, (O.transcode(stream(name)) if whole else S.encode(*planes)), mode, o


def expected(name, spec, sei=0):
    m = _model(name, key(spec), sei)
    return None if m is None else m[2]


def assert_planes(got, exp, what):
    for g, e, pl in zip(got, exp, "YUV"):
        assert g.shape == e.shape, (what, pl, g.shape, e.shape)
        diff = np.argwhere(g != e)
        assert diff.size == 0, f"{what} {pl}: {len(diff)} mismatches, first at {diff[:5].tolist()}, " \
                               f"got {g[tuple(diff[0])]} expected {e[tuple(diff[0])]}"


# 1. planes, through decode_multi4 with the case's renditions in flight
@pytest.mark.parametrize("case", range(len(CASES)))
def test_oriented_planes_bit_exact(engine, case):
    name, specs = CASES[case]
    for pick, spec in enumerate(specs):
        win, planes, _, mode, o = _model(name, key(spec))
        y, u, v, size, m, w, ro, so = engine.decode_multi4(stream(name), specs, pick)
        levels = {_model(name, key(s))[3] for s in specs if _model(name, key(s))[0] == win and _model(name, key(s))[4] == o} & {1, 2, 3}
        want_mode = 5 if mode in (1, 2, 3) and len(levels) > 1 else mode
        assert (m, w, size, ro, so) == (want_mode, win, (planes[0].shape[1], planes[0].shape[0]), o, 0), (name, spec, m, w, size, ro)
        assert_planes((y, u, v), planes, f"{name} {spec}")


# 2. files: every case in one batch, with plain items among them
def test_oriented_jpegs_one_batch_byte_exact(engine):
    items = [(n, list(specs)) for n, specs in CASES] + [(P11, [0]), (A13, [0, 1]), (P01, [0])]
    outs = engine.transcode_multi([stream(n) for n, _ in items], [specs for _, specs in items])
    bad = [(n, sp) for (n, specs), o in zip(items, outs) for sp, got in zip(specs, o) if got != expected(n, sp)]
    assert not bad, bad[:8]
    assert all(st == 0 for row in engine.last_status for st in row)
    assert outs[-3] == [O.transcode(stream(P11))] and outs[-1] == [O.transcode(stream(P01))] and outs[-2][0] == O.transcode(stream(A13))
    # SOF0 carries the oriented output size
    assert O.jpeg_parse(outs[5][3])[:2] == (240, 416) and O.jpeg_parse(outs[5][1])[:2] == (416, 240)
    assert O.jpeg_parse(outs[13][0])[:2] == (100, 150) and O.jpeg_parse(outs[13][2])[:2] == (64, 64)
    # the keyword form: one rendition per item
    got = engine.transcode([stream(P01), stream(P11), stream(P12)], orient=[6, None, 3], scale=[1, 0, 0])
    assert got == [expected(P01, ori(6, scale=1)), O.transcode(stream(P11)), expected(P12, ori(3))] and engine.last_status == [0, 0, 0]


# 3. one full-size picture
def test_oriented_1080p(engine):
    rend = [ori(6), ori(6, cover=(256, 256))]
    outs = engine.transcode_multi([stream(IMG)], rend)[0]
    assert [O.jpeg_parse(j)[:2] for j in outs] == [(1080, 1920), (256, 256)]
    assert _model(IMG, key(rend[1]))[0] == (0, 420, 1080, 1080)
    assert outs == [expected(IMG, sp) for sp in rend]


# 4. sharing: renditions of one orientation share its oriented source; rendition 0 stays the plain picture
def test_renditions_share_an_orientation(engine):
    rend = [ori(6), ori(6, scale=1), ori(6, crop=(16, 16, 64, 96)), ori(6), ori(6, fit=(120, 208))]
    outs = engine.transcode_multi([stream(P01)], rend)[0]
    assert outs == [expected(P01, sp) for sp in rend] and outs[0] == outs[3] and outs[1] == outs[4]
    st = engine.stats()
    assert (st["frames"], st["renditions"]) == (1, 5)
    rend = [0, ori(6), ori(3, scale=1)]
    outs = engine.transcode_multi([stream(P01), stream(P12)], rend)
    assert outs[0] == [O.transcode(stream(P01)), expected(P01, rend[1]), expected(P01, rend[2])]
    assert outs[1] == [O.transcode(stream(P12)), expected(P12, rend[1]), expected(P12, rend[2])]
    assert engine.stats()["renditions"] == 6
    # orient 0 and 1 are the plain rendition, byte for byte
    outs = engine.transcode_multi([stream(P01)], [ori(0), ori(1), 0, ori(1, scale=1), 1])[0]
    assert outs[0] == outs[1] == outs[2] == O.transcode(stream(P01)) and outs[3] == outs[4]


# 5. algebra on the planes the GPU made
def test_orientation_algebra(engine):
    for name in (P12, P08):
        y0, u0, v0 = engine.decode_multi4(stream(name), [ori(0)], 0)[:3]
        y3, u3, v3 = engine.decode_multi4(stream(name), [ori(3)], 0)[:3]
        assert_planes((y3, u3, v3), [p[::-1, ::-1] for p in (y0, u0, v0)], f"{name} 180")
        y6, u6, v6 = engine.decode_multi4(stream(name), [ori(6)], 0)[:3]
        back = OR.orient_planes(y6, u6, v6, 8)
        assert OR.inverse(6) == 8
        assert_planes(back, (y0, u0, v0), f"{name} 6 then 8")


# 6. auto: the stream's display orientation SEI
def test_auto_orientation(engine):
    cases = [(P11, 265, 0, 0, 3), (P12, 265, 1, 0, 0), (A12, 264, 0, 1, 1), (A12, 264, 0, 0, 1), (P01, 265, 1, 1, 1)]
    ss, want_auto, want_plain, seis = [], [], [], []
    for name, codec, hor, ver, k in cases:
        o = OR.sei_orient(hor, ver, k)
        ss.append(OR.insert_sei(stream(name), codec, hor, ver, k))
        seis.append(o)
        want_auto.append([expected(name, ori(o)), expected(name, ori(o, scale=1))])
        want_plain.append([O.transcode(stream(name)), expected(name, 1)])
    assert seis == [6, 2, 7, 8, 6]
    auto = engine.transcode_multi(ss, [ori("auto"), ori("auto", scale=1)])
    assert auto == want_auto and all(st == 0 for row in engine.last_status for st in row)
    assert engine.transcode_multi(ss, [0, 1]) == want_plain  # the SEI is never applied unasked
    assert engine.transcode(ss) == [w[0] for w in want_plain]
    # an explicit orientation ignores the SEI; auto on a stream without it is the plain picture
    assert engine.transcode([ss[0], stream(P11)], orient=[3, "auto"]) == [expected(P11, ori(3)), O.transcode(stream(P11))]
    info = engine.decode_multi4(ss[2], [ori("auto")], 0)
    assert info[3:] == ((40, 72), 0, (0, 0, 40, 72), 7, 7)
    assert engine.decode_multi4(ss[2], [0, ori(2)], 1)[6:] == (2, 7)


# 7. the asynchronous path, two batches in flight
def test_async_batches(engine):
    names = [P01, A13, P11, A31, P08, P19, P12, A12, P25]
    opts = [0, ori(6), ori(3, scale=1), ori(5, crop=(2, 6, 30, 40)), ori(2), 1]
    batches = [[names[(i + 3 * b) % len(names)] for i in range(12)] for b in range(2)]
    specs = [[opts[i % len(opts)]] for i in range(12)]
    res = engine.transcode_multi_async([[stream(n) for n in bn] for bn in batches], specs)
    assert all(st == 0 for batch in engine.last_status for row in batch for st in row)
    for bn, outs in zip(batches, res):
        for n, s, o in zip(bn, specs, outs):
            assert o == [expected(n, s[0])], (n, s)
    kw = engine.transcode_async([[stream(P01), stream(P11)], [stream(A13)]], orient=[[8, None], "auto"], scale=[[1, 0], 1])
    assert kw == [[expected(P01, ori(8, scale=1)), O.transcode(stream(P11))], [expected(A13, 1)]]


# 8. the facade, from two threads with different orientations
def test_facade_multi4_from_threads(engine):
    import h2j
    lib = h2j.load_library()
    jobs = [(P01, [ori(6, scale=1), 0, ori(9)]), (A13, [ori(3), ori(5, fit=(100, 0))])]
    got = {}

    def call(i, name, specs):
        s = stream(name)
        buf = (ctypes.c_uint8 * len(s)).from_buffer_copy(s)
        n = len(specs)
        opts = (h2j.OutOpts4 * n)(*[h2j.OutOpts4(*(tuple(h2j.rendition_spec(sp)) + (0,) * 5)[:10]) for sp in specs])
        jpeg = (ctypes.POINTER(ctypes.c_uint8) * n)()
        lens, status = (ctypes.c_size_t * n)(), (ctypes.c_int * n)()
        rc = lib.h2j_h265_to_jpeg_mem_multi4(buf, len(s), n, opts, jpeg, lens, status)
        out = [ctypes.string_at(jpeg[r], lens[r]) if status[r] == 0 else None for r in range(n)]
        for r in range(n):
            if jpeg[r]:
                lib.h2j_free(jpeg[r])
        got[i] = (rc, [status[r] for r in range(n)], out)

    ts = [threading.Thread(target=call, args=(i, n, sp)) for i, (n, sp) in enumerate(jobs)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for i, (n, specs) in enumerate(jobs):
        rc, st, out = got[i]
        want = [expected(n, sp) for sp in specs]
        assert rc == 0 and st == [0 if w is not None else h2j.ERR_OUT_OPTS for w in want], (n, rc, st)
        assert out == want, n


# 9. invalid orientations fail alone
def test_invalid_orientation_fails_alone(engine):
    import h2j
    outside = ori(8, crop=(36, 10, 300, 200))  # inside the decoded 416 x 240 picture, outside the oriented 240 x 416 one
    rend = [0, ori(9), ori(6), ori(-2), outside, ori(8, crop=(36, 10, 200, 300))]
    for b in (rend[1], rend[3], outside):
        assert expected(P01, b) is None
    outs = engine.transcode_multi([stream(P01), stream(P11)], [rend, [ori(6)]])
    assert engine.last_status == [[0, h2j.ERR_OUT_OPTS, 0, h2j.ERR_OUT_OPTS, h2j.ERR_OUT_OPTS, 0], [0]]
    assert outs[0] == [expected(P01, sp) for sp in rend] and outs[1] == [expected(P11, ori(6))]
    assert "orient 9" in engine.frame_error(1) and "orient -2" in engine.frame_error(3)
    msg = engine.frame_error(4)
    assert "the picture is 240 x 416 at orientation 8" in msg and "crop 36, 10, 300 x 200" in msg, msg
    assert engine.frame_error(0) == "" and engine.frame_error(2) == ""
    # non-zero reserved, through the C call
    lib = h2j.load_library()
    s = stream(P11)
    buf = (ctypes.c_uint8 * len(s)).from_buffer_copy(s)
    ptrs = (ctypes.POINTER(ctypes.c_uint8) * 1)(ctypes.cast(buf, ctypes.POINTER(ctypes.c_uint8)))
    sizes, nr = (ctypes.c_size_t * 1)(len(s)), (ctypes.c_int32 * 1)(3)
    opts = (h2j.OutOpts4 * 3)(h2j.OutOpts4(orient=6), h2j.OutOpts4(orient=6, reserved=(ctypes.c_int32 * 6)(0, 0, 0, 0, 0, 1)),
                              h2j.OutOpts4(reserved=(ctypes.c_int32 * 6)(0, 0, 0, 7, 0, 0)))
    cap = 1 << 20
    out = (ctypes.c_uint8 * cap)()
    offs, lens, status = (ctypes.c_size_t * 3)(), (ctypes.c_size_t * 3)(), (ctypes.c_int * 3)()
    rc = lib.h2j_engine_transcode_multi4(engine._h, 1, ptrs, sizes, nr, opts, out, cap, offs, lens, status)
    assert rc == 0 and list(status) == [0, h2j.ERR_OUT_OPTS, h2j.ERR_OUT_OPTS]
    assert bytes(out[offs[0]:offs[0] + lens[0]]) == expected(P11, ori(6))
