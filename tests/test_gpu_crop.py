"""GPU: crop and cover -- JPEGs of a window of the picture (DESIGN.md "Crop and cover").

The one definition: a windowed rendition's bytes are those the same call returns for a picture whose cropped
planes are the window's samples.  So every expected value is the oracle's decoded planes sliced with numpy,
through the existing models (scale_ref.scale_planes, resize_ref.resize_planes, scale_ref.encode) -- no new
arithmetic, and never another call into the engine.  The window and cover rule is tests/crop_ref.py's."""
import ctypes
import functools
import threading

import numpy as np
import pytest

import crop_ref as C
import oracle_py as O
import resize_ref as R
import scale_ref as S
from conftest import golden, read

pytestmark = pytest.mark.gpu

P01 = "hevc/p01_416x240_q22.h265"  # SAO on, 416 = 26 x 16
P07 = "hevc/p07_336x200_q45.h265"  # SAO on, 336 = 21 x 16, textured: its windows' variance sums reach other quantisers
P11 = "hevc/p11_64x64_tiny.h265"
P12 = "hevc/p12_72x40_odd_crop.h265"
A12 = "h264/a12_72x40_odd_crop.h264"
P15 = "hevc/p15_48x200_wpp_narrow.h265"
P19 = "hevc/p19_480x272_tiles2x2_wpp_nolf.h265"
P25 = "hevc/p25_400x240_conf_left64_top16.h265"
P08 = "hevc/p08_320x180_10bit_q2.h265"
P27 = "hevc/p27_416x240_12bit.h265"
A13 = "h264/a13_320x180_10bit_q0.h264"
A31 = "h264/a31_336x192_mbaff_cabac_8x8.h264"
A37 = "h264/a37_320x192_paff_cabac_8x8_slices.h264"
IMG = "img01.h264"  # 1920 x 1080

WA, WB = (36, 10, 300, 200), (2, 6, 44, 36)  # luma origin 4 mod 16, chroma 2 mod 8; an odd chroma origin
WC = (416 - 44, 240 - 36, 44, 36)            # ends in the picture's bottom-right corner
WH = (6, 4, 250, 150)                        # 16-bit samples: the chroma origin is 6 bytes
WD, WE = (24, 10, 300, 200), (22, 6, 300, 200)  # byte offsets 8 / 12 (luma / chroma) and 6 / 11: the remaining dword
                                                # offsets of a 16-byte load, and a byte shift of 3


def crop(win, **kw):
    return dict(crop=win, **kw)


def levels(win):
    return [crop(win, scale=k) for k in (1, 2, 3)]


# (vector, renditions): the smallest shapes that reach each way a window can go wrong
CASES = [
    (P11, [crop((0, 0, 64, 64)), crop((0, 0, 0, 0)), crop((16, 16, 32, 32)), crop((2, 2, 2, 2))]),
    (P01, levels(WA) + levels(WB)),          # shifted lanes, edge lanes, real samples right of and below the window
    (P01, levels(WC) + [crop(WA, fit=(290, 0)), crop(WA, fit=(100, 0)), crop(WA, fit=(30, 0))]),  # K3r: ratios 1+, 3, 10
    (P12, [crop((2, 2, 60, 30), scale=1)]),  # chroma pitch 36: the single-sample path
    (A12, [crop((2, 2, 60, 30), scale=1)]),
    (P25, [crop((6, 4, 200, 120), scale=1), crop((6, 4, 200, 120), fit=(150, 0))]),  # conformance crop + window
    (P08, levels(WH) + [crop(WH, fit=(100, 0))]),
    (P27, levels(WH) + [crop(WH, fit=(100, 0))]),
    (A13, levels(WH) + [crop(WH, fit=(100, 0))]),
    (A31, [crop((10, 6, 200, 100), scale=1)]),
    (A37, [crop((10, 6, 200, 100), scale=1)]),
    (P19, [crop(WA, scale=2)]),              # pic2 == pic
    (P01, levels(WD) + levels(WE)),
]


@functools.lru_cache(maxsize=None)
def stream(name):
    return read(golden(name))


@functools.lru_cache(maxsize=None)
def decoded(name):
    return O.decode(stream(name), S.codec_of(name))


def size_of(name):
    y = decoded(name)[0]
    return y.shape[1], y.shape[0]


def key(spec):
    return spec if isinstance(spec, int) else tuple(sorted(spec.items()))


@functools.lru_cache(maxsize=None)
def _model(name, k):
    """(window, 8-bit planes or None for the whole unscaled picture, JPEG bytes); None: invalid options."""
    spec = k if isinstance(k, int) else dict(k)
    y, u, v, bd = decoded(name)
    W, H = size_of(name)
    r = C.resolve(W, H, **C.spec_fields(spec))
    if r is None:
        return None
    win, (ow, oh), mode = r
    wy, wu, wv = C.window_planes(y, u, v, win)
    if mode == C.RESAMPLE:
        planes = R.resize_planes(wy, wu, wv, bd, ow, oh)
    else:
        planes = S.scale_planes(wy, wu, wv, bd, mode)  # mode 0: the 8-bit conversion alone
    assert planes[0].shape == (oh, ow)
    whole = win == (0, 0, W, H) and mode == 0
    return win, planes, (O.transcode(stream(name)) if whole else S.encode(*planes)), mode


def expected(name, spec):
    m = _model(name, key(spec))
    return None if m is None else m[2]


def assert_planes(got, exp, what):
    for g, e, pl in zip(got, exp, "YUV"):
        assert g.shape == e.shape, (what, pl, g.shape, e.shape)
        diff = np.argwhere(g != e)
        assert diff.size == 0, f"{what} {pl}: {len(diff)} mismatches, first at {diff[:5].tolist()}, " \
                               f"got {g[tuple(diff[0])]} expected {e[tuple(diff[0])]}"


# 1. planes, through decode_multi3 with the rendition alone in flight
@pytest.mark.parametrize("case", range(len(CASES)))
def test_window_planes_bit_exact(engine, case):
    name, specs = CASES[case]
    for spec in specs:
        win, planes, _, mode = _model(name, key(spec))
        y, u, v, size, m, w = engine.decode_multi3(stream(name), [spec], 0)
        assert (m, w, size) == (mode, win, (planes[0].shape[1], planes[0].shape[0])), (name, spec, m, w, size)
        assert_planes((y, u, v), planes, f"{name} {spec}")


# 2. files: every case in one batch
def test_window_jpegs_one_batch_byte_exact(engine):
    outs = engine.transcode_multi([stream(n) for n, _ in CASES], [specs for _, specs in CASES])
    bad = [(n, sp) for (n, specs), o in zip(CASES, outs) for sp, got in zip(specs, o) if got != expected(n, sp)]
    assert not bad, bad[:8]
    assert all(st == 0 for row in engine.last_status for st in row)
    # whole-picture windows give the plain call's bytes; SOF0 carries the output size
    assert outs[0][0] == outs[0][1] == O.transcode(stream(P11))
    assert O.jpeg_parse(outs[0][3])[:2] == (2, 2) and O.jpeg_parse(outs[1][2])[:2] == (38, 26)
    # the keyword form: one rendition per item
    got = engine.transcode([stream(P01), stream(P11)], crop=[WA, None], scale=[2, 0])
    assert got == [expected(P01, crop(WA, scale=2)), O.transcode(stream(P11))] and engine.last_status == [0, 0]


# 3. the variance-fold trap: an unscaled 16-aligned window of a picture whose MB variances K3 SAO sums
def _var_sum(y8):
    y8 = np.ascontiguousarray(y8, dtype=np.uint8)
    v = ctypes.c_int64(0)
    fn = O.lib().oracle_jpeg_qscale
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.POINTER(ctypes.c_uint8), ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p]
    fn(y8.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), y8.shape[1], y8.shape[0], y8.shape[1], ctypes.byref(v), None)
    return v.value


def _qscale(var_sum):
    fn = O.lib().oracle_jpeg_qscale_from_var
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int64, ctypes.c_void_p]
    return fn(var_sum, None)


def test_unscaled_aligned_window_of_sao_picture(engine):
    w16 = (16, 16, 160, 96)
    win, small = crop(w16), crop((16, 16, 96, 96))
    # the picture qualifies: 8-bit, width a multiple of 16, and SAO is on and acts (the deblocked picture is not
    # the decoded one), so K3 SAO folds the whole picture's variance sum into the frame's jstat
    y, u, v, bd = decoded(P07)
    assert bd == 8 and y.shape[1] % 16 == 0
    assert any(not np.array_equal(a, b) for a, b in zip(engine.decode(stream(P07), 2)[:3], engine.decode(stream(P07), 0)[:3]))
    # only the quantiser scale enters the file, so the test can see a wrong sum only where it changes the scale:
    # the window's differs from that of no sum at all (K4a skipped), of the whole picture's sum (the frame's
    # jstat inherited) and of both (K4a adding to SAO's fold)
    for ww in (w16, small["crop"]):
        vw, vp = _var_sum(C.window_planes(y, u, v, ww)[0]), _var_sum(y)
        assert len({_qscale(vw), _qscale(0), _qscale(vp), _qscale(vp + vw)}) == 4, (ww, vw, vp)
    want = expected(P07, win)
    assert O.jpeg_parse(want)[:2] == (160, 96)
    alone = engine.transcode_multi([stream(P07)], [win])[0]
    assert alone == [want]
    beside = engine.transcode_multi([stream(P07), stream(P11)], [[win, 0], [0]])
    assert beside[0] == [want, O.transcode(stream(P07))] and beside[1] == [O.transcode(stream(P11))]
    first = engine.transcode_multi([stream(P07)], [0, win, small])[0]
    assert first == [O.transcode(stream(P07)), want, expected(P07, small)]
    two = engine.transcode_multi([stream(P07)], [small, win])[0]  # two windows, no whole picture
    assert two == [expected(P07, small), want]
    yy, uu, vv, size, mode, w = engine.decode_multi3(stream(P07), [win], 0)
    assert (size, mode, w) == ((160, 96), 0, w16)
    assert_planes((yy, uu, vv), _model(P07, key(win))[1], "unscaled window")


# 4. K3p: pyramids are per window
def test_pyramids_per_window(engine):
    rend = [crop(WA, scale=1), crop(WA, scale=2), crop(WA, scale=3), crop(WB, scale=1), crop(WB, scale=2), 0, 1]
    outs = engine.transcode_multi([stream(P01)], rend)[0]
    assert outs == [expected(P01, sp) for sp in rend]
    for pick, sp in enumerate(rend):
        y, u, v, size, mode, w = engine.decode_multi3(stream(P01), rend, pick)
        assert mode == (0 if sp == 0 else 1 if sp == 1 else 5), (pick, mode)  # A's and B's levels: K3p; the whole picture's: K3s
        assert_planes((y, u, v), _model(P01, key(sp))[1], f"pick {pick}")
    singles = [engine.transcode([stream(P01)], crop=sp["crop"], scale=sp["scale"])[0] if isinstance(sp, dict)
               else engine.transcode([stream(P01)], scale=sp)[0] for sp in rend]
    assert singles == outs
    # renditions that resolve to the same (window, output) share a view
    dup = engine.transcode_multi([stream(P01)], [crop(WA, scale=1), crop(WA, fit=(150, 100)), crop(WA, max_dim=150)])[0]
    assert dup[0] == dup[1] == dup[2] == expected(P01, crop(WA, scale=1))


# 5. cover
def test_cover_1080p(engine):
    rend = [0, {"cover": (540, 540)}, {"cover": (270, 270)}, {"cover": (256, 256)}, {"cover": (640, 360)}]
    outs = engine.transcode_multi([stream(IMG)], rend)[0]
    assert [O.jpeg_parse(j)[:2] for j in outs] == [(1920, 1080), (540, 540), (270, 270), (256, 256), (640, 360)]
    sq = (420, 0, 1080, 1080)
    assert outs[0] == O.transcode(stream(IMG))
    assert outs[1] == expected(IMG, crop(sq, scale=1)) == expected(IMG, rend[1])
    assert outs[2] == expected(IMG, crop(sq, scale=2)) == expected(IMG, rend[2])
    assert outs[3] == expected(IMG, rend[3]) and _model(IMG, key(rend[3]))[3] == C.RESAMPLE  # the K3r model
    assert outs[4] == expected(IMG, {"fit": (640, 360)})
    modes = [engine.decode_multi3(stream(IMG), rend, p)[4:] for p in (1, 2, 3)]
    assert modes == [(5, sq), (5, sq), (4, sq)]  # 540 and 270: two levels of one window, one K3p read
    assert engine.transcode([stream(IMG)], cover=(256, 256)) == [outs[3]]


def test_cover_narrow_picture(engine):
    out = engine.transcode([stream(P15)], cover=(16, 16))[0]
    assert _model(P15, key({"cover": (16, 16)}))[0] == (0, 76, 48, 48)
    assert out == expected(P15, {"cover": (16, 16)}) and O.jpeg_parse(out)[:2] == (16, 16)


# 6. invalid options fail alone
def _raw_multi3(engine, streams, nrend, opts_flat):
    import h2j
    lib = h2j.load_library()
    n, total = len(streams), len(opts_flat)
    bufs = [(ctypes.c_uint8 * len(s)).from_buffer_copy(s) for s in streams]
    ptrs = (ctypes.POINTER(ctypes.c_uint8) * n)(*[ctypes.cast(b, ctypes.POINTER(ctypes.c_uint8)) for b in bufs])
    sizes = (ctypes.c_size_t * n)(*[len(s) for s in streams])
    nr = (ctypes.c_int32 * n)(*nrend)
    opts = (h2j.OutOpts3 * total)(*opts_flat)
    cap = 4 << 20
    out = (ctypes.c_uint8 * cap)()
    offs, lens, status = (ctypes.c_size_t * total)(), (ctypes.c_size_t * total)(), (ctypes.c_int * total)()
    rc = lib.h2j_engine_transcode_multi3(engine._h, n, ptrs, sizes, nr, opts, out, cap, offs, lens, status)
    return rc, [status[i] for i in range(total)], [bytes(out[offs[i]:offs[i] + lens[i]]) for i in range(total)]


def test_invalid_window_fails_alone(engine):
    import h2j
    bad = [crop((3, 0, 0, 0)), crop((0, 0, 33, 32)), crop((400, 0, 32, 32)), crop((0, 240, 0, 0)), crop((-2, 0, 0, 0)),
           crop((0, 0, 0, -4)), {"cover": (16, 16), "stretch": True}, {"cover": (16, 0)}, {"cover": (16, 16), "scale": 1}]
    good = [0, crop(WA, scale=1), {"cover": (64, 64)}]
    for b in bad:
        assert expected(P01, b) is None, b  # the model agrees that it is invalid
    items = [[good[0], bad[0], bad[1], good[1], bad[2], bad[3]], [0], [bad[4], bad[5], good[2], bad[6], bad[7], bad[8], 1]]
    names = [P01, P11, P01]
    outs = engine.transcode_multi([stream(n) for n in names], items)
    o = 0
    for n, specs, row, sts in zip(names, items, outs, engine.last_status):
        for sp, got, st in zip(specs, row, sts):
            msg = engine.frame_error(o)
            o += 1
            if any(sp is b for b in bad):
                assert got is None and st == h2j.ERR_OUT_OPTS and "the picture is 416 x 240" in msg, (sp, st, msg)
            else:
                assert st == 0 and msg == "" and got == expected(n, sp), (n, sp, st)
    # non-zero reserved, through the C call
    mk = lambda **kw: h2j.OutOpts3(**kw)
    rc, st, got = _raw_multi3(engine, [stream(P11), stream(P01)], [2, 2],
                              [mk(), mk(crop_x=16, crop_y=16, crop_w=32, crop_h=32, reserved=(ctypes.c_int32 * 3)(0, 0, 1)),
                               mk(crop_x=36, crop_y=10, crop_w=300, crop_h=200, scale_log2=1), mk(reserved=(ctypes.c_int32 * 3)(5, 0, 0))])
    assert rc == 0 and st == [0, h2j.ERR_OUT_OPTS, 0, h2j.ERR_OUT_OPTS]
    assert engine.frame_error(1) and engine.frame_error(3) and engine.frame_error(0) == ""
    assert got[0] == O.transcode(stream(P11)) and got[2] == expected(P01, crop(WA, scale=1))


# 6b. a rendition that fails only after the parse, with no valid sibling in its item
def test_item_with_every_window_outside_the_picture(engine):
    import h2j
    out = (100, 0, 32, 32)  # of the 64 x 64 picture
    got = engine.transcode([stream(P11)], crop=out)  # alone: the batch has no frame
    assert got == [None] and engine.last_status == [h2j.ERR_OUT_OPTS] and "the picture is 64 x 64" in engine.frame_error(0)
    got = engine.transcode([stream(P01), stream(P11), stream(A12)], crop=[None, out, None])  # between good items
    assert got == [O.transcode(stream(P01)), None, O.transcode(stream(A12))]
    assert engine.last_status == [0, h2j.ERR_OUT_OPTS, 0] and engine.frame_error(1) and engine.frame_error(2) == ""
    rend = [[crop(out), crop((0, 80, 0, 0), scale=1), crop((60, 60, 8, 8), fit=(2, 2))], [crop((2, 2, 60, 30), scale=1), 0]]
    outs = engine.transcode_multi([stream(P11), stream(P12)], rend)  # every rendition of a multi-rendition item
    assert outs == [[None] * 3, [expected(P12, rend[1][0]), O.transcode(stream(P12))]]
    assert engine.last_status == [[h2j.ERR_OUT_OPTS] * 3, [0, 0]]
    st = engine.stats()
    assert (st["parsed"], st["frames"], st["renditions"]) == (2, 1, 2)
    res = engine.transcode_async([[stream(P11)], [stream(P11), stream(P12)]], crop=[out, [out, (2, 2, 60, 30)]])
    assert res == [[None], [None, expected(P12, crop((2, 2, 60, 30)))]]
    assert engine.transcode([stream(P11)]) == [O.transcode(stream(P11))]  # the engine goes on


# 7. the asynchronous path
def test_async_batches_cycling_options(engine):
    names = [P01, A13, P11, A31, P08, P19, P12, A12, P25]
    opts = [0, crop((16, 8, 32, 32)), {"cover": (32, 32)}, crop((6, 4, 52, 30), scale=1)]
    batches = [[names[(i + 2 * b) % len(names)] for i in range(12)] for b in range(3)]
    specs = [[opts[i % 4]] for i in range(12)]  # per item, the same in every batch (the streams differ)
    res = engine.transcode_multi_async([[stream(n) for n in bn] for bn in batches], specs)
    assert all(st == 0 for batch in engine.last_status for row in batch for st in row)
    plain = engine.transcode_multi_async([[stream(n) for n in bn] for bn in batches], [0])
    for bn, outs, pl in zip(batches, res, plain):
        for n, s, o, p in zip(bn, specs, outs, pl):
            assert o == [expected(n, s[0])], (n, s)
            if s[0] == 0:
                assert o == p  # the un-windowed items: the bytes of a run without any window in the batch
    # the keyword form, one entry per batch
    kw = engine.transcode_async([[stream(P01), stream(P11)], [stream(A13)]], crop=[[WA, None], (6, 4, 52, 30)], scale=[[1, 0], 1])
    assert kw == [[expected(P01, crop(WA, scale=1)), O.transcode(stream(P11))], [expected(A13, crop((6, 4, 52, 30), scale=1))]]


# 8. the facade, from four threads with different windows
def test_facade_multi3_from_threads(engine):
    import h2j
    lib = h2j.load_library()
    jobs = [(P01, [crop(WA, scale=1), 0]), (P01, [crop(WB, scale=2), {"cover": (64, 64)}]), (A13, [crop(WH, fit=(100, 0))]),
            (P11, [crop((16, 16, 32, 32)), crop((3, 0, 0, 0)), 1])]
    got = {}

    def call(i, name, specs):
        s = stream(name)
        buf = (ctypes.c_uint8 * len(s)).from_buffer_copy(s)
        n = len(specs)
        opts = (h2j.OutOpts3 * n)(*[h2j.OutOpts3(*(h2j.rendition_spec(sp) + (0, 0, 0, 0))[:9]) for sp in specs])
        jpeg = (ctypes.POINTER(ctypes.c_uint8) * n)()
        lens, status = (ctypes.c_size_t * n)(), (ctypes.c_int * n)()
        rc = lib.h2j_h265_to_jpeg_mem_multi3(buf, len(s), n, opts, jpeg, lens, status)
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
