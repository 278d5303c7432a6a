"""GPU: renditions -- several JPEGs of one picture from one parse and one reconstruction, the K3s
levels of a picture from one read (K3p).  Rendition r of an item is byte for byte the single-item
output with the same options, so every expected value comes from the models of those outputs
(tests/scale_ref.py, tests/resize_ref.py, oracle_py), never from another call into the engine."""
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

# the smallest vectors that reach each path of K3p
VECTORS = [
    "hevc/p11_64x64_tiny.h265",                 # one workgroup, 8x8 at k = 3
    "hevc/p12_72x40_odd_crop.h265",             # unaligned path; level sizes 36x20 / 18x10 / 10x6 do not nest
    "h264/a12_72x40_odd_crop.h264",
    "hevc/p15_48x200_wpp_narrow.h265",          # bottom clamp
    "hevc/p09_200x120_noqpd_notskip.h265",      # right clamp
    "hevc/p25_400x240_conf_left64_top16.h265",  # aligned non-zero crop
    "hevc/p01_416x240_q22.h265",                # SAO, variance fold
    "hevc/p19_480x272_tiles2x2_wpp_nolf.h265",  # SAO off
    "hevc/p08_320x180_10bit_q2.h265",           # 10-bit
    "hevc/p27_416x240_12bit.h265",              # 12-bit
    "h264/a29_192x112_14bit_cavlc_pcm.h264",    # 14-bit
    "h264/a45_208x128_mono_lossless.h264",      # mono
    "h264/a31_336x192_mbaff_cabac_8x8.h264",    # MBAFF
]
LEVEL_SETS = [(1, 2, 3), (1, 2), (1, 3), (2, 3)]
P11, P12 = VECTORS[0], VECTORS[1]


@functools.lru_cache(maxsize=None)
def stream(name):
    return read(golden(name))


@functools.lru_cache(maxsize=None)
def decoded(name):
    return O.decode(stream(name), S.codec_of(name))


@functools.lru_cache(maxsize=None)
def size_of(name):
    y = decoded(name)[0]
    return y.shape[1], y.shape[0]


@functools.lru_cache(maxsize=None)
def scaled_planes(name, k):
    y, u, v, bd = decoded(name)
    return S.scale_planes(y, u, v, bd, k)


@functools.lru_cache(maxsize=None)
def expected(name, spec):
    """JPEG bytes of one rendition.  spec: an int (scale) or (fit_w, fit_h, stretch)."""
    if isinstance(spec, int):
        return O.transcode(stream(name)) if spec == 0 else S.encode(*scaled_planes(name, spec))
    y, u, v, bd = decoded(name)
    ow, oh = R.fit_size(y.shape[1], y.shape[0], (spec[0], spec[1]), spec[2])
    if (ow, oh) == (y.shape[1], y.shape[0]):
        return O.transcode(stream(name))
    return S.encode(*R.resize_planes(y, u, v, bd, ow, oh))


def to_spec(spec):
    """The model's spec -> what Engine.transcode_multi takes."""
    return spec if isinstance(spec, int) else {"fit": (spec[0], spec[1]), "stretch": spec[2]}


def check(items, outs, status=None):
    """items: [(name, [model specs])]; outs: transcode_multi's result."""
    bad = [(i, n, sp) for i, ((n, specs), o) in enumerate(zip(items, outs))
           for sp, got in zip(specs, o) if got != expected(n, sp)]
    assert not bad, bad[:8]
    assert [len(o) for o in outs] == [len(specs) for _, specs in items]


def assert_planes(got, exp, what):
    for g, e, pl in zip(got, exp, "YUV"):
        assert g.shape == e.shape, (what, pl, g.shape, e.shape)
        diff = np.argwhere(g != e)
        assert diff.size == 0, f"{what} {pl}: {len(diff)} mismatches, first at {diff[:5].tolist()}, " \
                               f"got {g[tuple(diff[0])]} expected {e[tuple(diff[0])]}"


# 1. pyramid planes
@pytest.mark.parametrize("name", VECTORS)
def test_pyramid_planes_bit_exact(engine, name):
    for levels in LEVEL_SETS:
        for pick, k in enumerate(levels):
            y, u, v, size, mode = engine.decode_multi(stream(name), list(levels), pick)
            assert mode == 5, (levels, k, mode)  # K3p wrote them
            assert size == S.scaled_size(*size_of(name), k)
            assert_planes((y, u, v), scaled_planes(name, k), f"{name} levels={levels} k={k}")


def test_pyramid_planes_large_picture(engine):
    for pick, k in enumerate((1, 2, 3)):
        y, u, v, size, mode = engine.decode_multi(stream("img01.h265"), [1, 2, 3], pick)
        assert mode == 5
        assert_planes((y, u, v), scaled_planes("img01.h265", k), f"img01.h265 k={k}")


def test_decode_multi_modes(engine):
    """One level among the renditions is K3s's, a fit K3r's, the unscaled rendition the picture."""
    s = stream(P12)
    w, h = size_of(P12)
    rend = [0, 2, (50, 0)]
    for pick, mode in enumerate((0, 2, 4)):
        y, u, v, size, m = engine.decode_multi(s, rend, pick)
        assert m == mode
    y, u, v, size, m = engine.decode_multi(s, rend, 1)
    assert_planes((y, u, v), scaled_planes(P12, 2), "k=2 beside other renditions")
    yy, uu, vv, bd = decoded(P12)
    ow, oh = R.fit_size(w, h, (50, 0), False)
    y, u, v, size, m = engine.decode_multi(s, rend, 2)
    assert size == (ow, oh)
    assert_planes((y, u, v), R.resize_planes(yy, uu, vv, bd, ow, oh), "fit beside other renditions")


# 2. JPEG bytes, one batch
def test_rendition_jpegs_one_batch_byte_exact(engine):
    items = []
    for n in VECTORS:
        w, h = size_of(n)
        items.append((n, [0, 1, 2, 3, (50, 0, False), (w - 2, h - 2, True)]))
    items.append(("img01.h264", [0, 3, (512, 512, False)]))
    outs = engine.transcode_multi([stream(n) for n, _ in items], [[to_spec(sp) for sp in specs] for _, specs in items])
    check(items, outs)
    assert all(st == 0 for row in engine.last_status for st in row)
    assert O.jpeg_parse(outs[-1][2])[:2] == (512, 288)
    assert O.jpeg_parse(outs[1][3])[:2] == (10, 6)


# 3. one parse
def test_one_parse_per_item(engine):
    names = [VECTORS[i % len(VECTORS)] for i in range(20)]
    streams = [stream(n) for n in names]
    outs = engine.transcode_multi(streams, [0, 1, 2, 3])
    st = engine.stats()
    n = len(names)
    assert (st["parsed"], st["frames"], st["renditions"]) == (n, n, 4 * n)
    check([(nm, [0, 1, 2, 3]) for nm in names], outs)
    # the same outputs asked for as a repeated stream list: every item is parsed on its own
    engine.transcode(streams * 4, scale=[k for k in range(4) for _ in names])
    st = engine.stats()
    assert (st["parsed"], st["frames"], st["renditions"]) == (4 * n, 4 * n, 4 * n)


# 4. one rendition per item is the single-output path
def test_single_rendition(engine):
    streams = [stream(n) for n in VECTORS]
    outs = engine.transcode_multi(streams, [0])
    assert [o[0] for o in outs] == [O.transcode(s) for s in streams]
    outs = engine.transcode_multi(streams, [2])
    assert [o[0] for o in outs] == [expected(n, 2) for n in VECTORS]
    st = engine.stats()
    assert (st["parsed"], st["frames"], st["renditions"]) == (len(VECTORS),) * 3


# 5. failures
def test_invalid_rendition_fails_alone(engine):
    import h2j
    outs = engine.transcode_multi([stream(P11), stream(P12)], [[0, {"scale": 7}, 2, 3], [{"max_dim": -1}, 1]])
    assert engine.last_status == [[0, h2j.ERR_OUT_OPTS, 0, 0], [h2j.ERR_OUT_OPTS, 0]]
    assert outs[0][1] is None and outs[1][0] is None
    assert engine.frame_error(1) and engine.frame_error(4)
    assert engine.frame_error(0) == "" and engine.frame_error(5) == ""
    assert [outs[0][0], outs[0][2], outs[0][3], outs[1][1]] == \
           [expected(P11, 0), expected(P11, 2), expected(P11, 3), expected(P12, 1)]
    # every rendition invalid: the item is not parsed
    outs = engine.transcode_multi([stream(P11), stream(P12)], [[4, 5], [0, 1]])
    assert outs[0] == [None, None] and engine.last_status[0] == [h2j.ERR_OUT_OPTS] * 2
    assert outs[1] == [expected(P12, 0), expected(P12, 1)]
    assert engine.stats()["parsed"] == 1


def test_truncated_stream_fails_every_rendition(engine):
    streams = [stream(P11), stream(P12)[:16], stream(VECTORS[6])]
    outs = engine.transcode_multi(streams, [0, 1, 3])
    assert outs[1] == [None, None, None]
    assert len(set(engine.last_status[1])) == 1 and engine.last_status[1][0] < 0
    assert engine.frame_error(3) and engine.frame_error(3) == engine.frame_error(5)
    check([(P11, [0, 1, 3])], outs[:1])
    check([(VECTORS[6], [0, 1, 3])], outs[2:])
    assert engine.last_status[0] == [0, 0, 0] and engine.last_status[2] == [0, 0, 0]


def _raw_multi(engine, streams, nrend, opts_flat, cap):
    import h2j
    lib = h2j.load_library()
    n, total = len(streams), max(1, len(opts_flat))
    bufs = [(ctypes.c_uint8 * len(s)).from_buffer_copy(s) for s in streams]
    ptrs = (ctypes.POINTER(ctypes.c_uint8) * n)(*[ctypes.cast(b, ctypes.POINTER(ctypes.c_uint8)) for b in bufs])
    sizes = (ctypes.c_size_t * n)(*[len(s) for s in streams])
    nr = (ctypes.c_int32 * n)(*nrend)
    opts = (h2j.OutOpts2 * total)(*[h2j.OutOpts2(*h2j.rendition_spec(o)) for o in opts_flat])
    out = (ctypes.c_uint8 * cap)()
    offs, lens, status = (ctypes.c_size_t * total)(), (ctypes.c_size_t * total)(), (ctypes.c_int * total)()
    rc = lib.h2j_engine_transcode_multi(engine._h, n, ptrs, sizes, nr, opts, out, cap, offs, lens, status)
    t = lib.h2j_engine_submit_multi(engine._h, n, ptrs, sizes, nr, opts, out, cap, offs, lens, status) if rc == h2j.ERR_RENDITIONS else None
    return rc, t, [status[i] for i in range(total)], [bytes(out[offs[i]:offs[i] + lens[i]]) for i in range(total)]


def test_rendition_count_out_of_range(engine):
    import h2j
    s = stream(P11)
    for bad in (0, 9, -1):
        rc, t, _, _ = _raw_multi(engine, [s, s], [1, bad], [0] * 10, 1 << 20)
        assert rc == h2j.ERR_RENDITIONS and t == h2j.ERR_RENDITIONS, bad
    rc, _, st, outs = _raw_multi(engine, [s], [h2j.MAX_RENDITIONS], [0, 1, 2, 3, 0, 1, 2, 3], 1 << 20)
    assert rc == 0 and st == [0] * 8
    assert outs == [expected(P11, k) for k in (0, 1, 2, 3, 0, 1, 2, 3)]


def test_small_output_buffer_per_rendition(engine):
    name = VECTORS[6]
    sizes = [len(expected(name, k)) for k in (0, 1, 2, 3)]
    # room for the thumbnails, not for the full picture: the renditions are placed in order
    cap = sizes[0] - 1
    assert sizes[1] + sizes[2] + sizes[3] <= cap
    rc, _, st, outs = _raw_multi(engine, [stream(name)], [4], [0, 1, 2, 3], cap)
    assert rc == -3 and st == [-50, 0, 0, 0]
    assert outs[1:] == [expected(name, k) for k in (1, 2, 3)]
    res = engine.transcode_multi([stream(name)], [0, 1, 2, 3], out_cap=cap)  # the retry
    check([(name, [0, 1, 2, 3])], res)
    assert engine.last_status == [[0, 0, 0, 0]]


# 6. duplicates
def test_duplicate_renditions(engine):
    outs = engine.transcode_multi([stream(P11), stream(P12)], [[0, 0], [1, (36, 20), {"max_dim": 36}, 1]])
    assert outs[0][0] == outs[0][1] == expected(P11, 0)
    assert outs[1][0] == outs[1][1] == outs[1][2] == outs[1][3] == expected(P12, 1)
    assert expected(P12, (36, 20, False)) == expected(P12, 1)  # the fit resolves to the 1/2 size
    st = engine.stats()
    assert (st["parsed"], st["frames"], st["renditions"]) == (2, 2, 6)


# 7. mixed layout
def test_mixed_rendition_counts_one_batch(engine):
    """Every parity vector, 1..4 renditions each drawn from {0, 1, 2, 3, fit}, and a large picture with
    (0, 1, 2, 3) in the middle: frames and views, K3s / K3p / K3r side by side, max_mcu over the views."""
    names = sorted("hevc/" + os.path.basename(p) for p in glob.glob(golden("hevc/*.h265"))) + \
            sorted("h264/" + os.path.basename(p) for p in glob.glob(golden("h264/*.h264")))
    assert len(names) >= 80
    pool = [0, 1, 2, 3, (50, 0, False)]
    items = [(n, [pool[(i + 2 * j) % 5] for j in range(i % 4 + 1)]) for i, n in enumerate(names)]
    items.insert(len(items) // 2, ("img01.h265", [0, 1, 2, 3]))
    outs = engine.transcode_multi([stream(n) for n, _ in items], [[to_spec(sp) for sp in specs] for _, specs in items])
    check(items, outs)
    st = engine.stats()
    assert st["parsed"] == st["frames"] == len(items)
    assert st["renditions"] == sum(len(specs) for _, specs in items)


# 8. more than 1024 views in one submit
def test_async_batches_beyond_1024_views(engine):
    names = VECTORS[:10]
    rend = [0, 1, 3, (50, 0, False)]
    batches = [[names[(i + 3 * b) % len(names)] for i in range(300 + b)] for b in range(2)]
    res = engine.transcode_multi_async([[stream(n) for n in b] for b in batches], [to_spec(sp) for sp in rend])
    for b, outs in zip(batches, res):
        check([(n, rend) for n in b], outs)
    assert all(st == 0 for batch in engine.last_status for row in batch for st in row)
    outs = engine.transcode([stream(n) for n in names])
    assert outs == [expected(n, 0) for n in names]


# 9. facade
def test_facade_multi_from_threads(engine):
    import h2j
    lib = h2j.load_library()
    jobs = [(P11, [0, 1, 2, 3]), (VECTORS[6], [3, 0]), (VECTORS[8], [1, 2, (50, 0, False)]), (P12, [(70, 38, True), 2, 2])]
    got = {}

    def call(i, name, specs):
        s = stream(name)
        buf = (ctypes.c_uint8 * len(s)).from_buffer_copy(s)
        n = len(specs)
        opts = (h2j.OutOpts2 * n)(*[h2j.OutOpts2(*h2j.rendition_spec(to_spec(sp))) for sp in specs])
        jpeg = (ctypes.POINTER(ctypes.c_uint8) * n)()
        lens, status = (ctypes.c_size_t * n)(), (ctypes.c_int * n)()
        rc = lib.h2j_h265_to_jpeg_mem_multi(buf, len(s), n, opts, jpeg, lens, status)
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
        assert rc == 0 and st == [0] * len(specs), (n, rc, st)
        assert out == [expected(n, sp) for sp in specs], n
    s = stream(P11)
    buf = (ctypes.c_uint8 * len(s)).from_buffer_copy(s)
    assert lib.h2j_h265_to_jpeg_mem_multi(buf, len(s), 0, None, None, None, None) == h2j.ERR_RENDITIONS
