"""Oriented output without a GPU: the option struct against the header, the pure h2j_crop_window4 and
h2j_stream_orientation of the C library against tests/orient_ref.py, and the Python spec parser."""
import ctypes
import os
import random
import re

import pytest

import crop_ref as C
import h2j
import orient_ref as O
from conftest import ROOT, golden, read

ERR = -60
HEVC, H264 = "hevc/p11_64x64_tiny.h265", "h264/a12_72x40_odd_crop.h264"


def c_resolve(W, H, orient=0, sei=0, scale=0, max_dim=0, fw=0, fh=0, flags=0, crop=(0, 0, 0, 0), reserved=(0,) * 6):
    lib = h2j.load_library()
    o = h2j.OutOpts4(scale, max_dim, fw, fh, flags, crop[0], crop[1], crop[2], crop[3], orient, (ctypes.c_int32 * 6)(*reserved))
    win, ow, oh, ro = (ctypes.c_int32 * 4)(7, 7, 7, 7), ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    rc = lib.h2j_crop_window4(W, H, ctypes.byref(o), sei, win, ctypes.byref(ow), ctypes.byref(oh), ctypes.byref(ro))
    if rc != 0:
        assert rc == ERR and list(win) == [7, 7, 7, 7] and (ow.value, oh.value, ro.value) == (-1, -1, -1)  # nothing written
        return None
    return tuple(win), (ow.value, oh.value), ro.value


def model(W, H, **kw):
    r = O.resolve(W, H, **kw)
    return None if r is None else (r[0], r[1], r[3])


def test_struct_and_constants_match_header():
    src = open(os.path.join(ROOT, "include", "h2j.h")).read()
    for name, val in (("H2J_ORIENT_AUTO", h2j.ORIENT_AUTO), ("H2J_ERR_NO_STAGE", h2j.ERR_NO_STAGE)):
        m = re.search(r"#define\s+" + name + r"\s+\((-?\d+)\)", src)
        assert m and int(m.group(1)) == val, name
    assert h2j.ORIENT_AUTO == O.AUTO == -1 and h2j.ERR_NO_STAGE == -62
    m = re.search(r"typedef struct \{([^}]*)\}\s*h2j_out_opts4;", src)
    assert m
    names = []
    for decl in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        assert decl.startswith("int32_t "), decl
        for nm in decl[len("int32_t "):].split(","):
            k = re.match(r"(\w+)\[(\d+)\]$", nm.strip())
            names += [(k.group(1), int(k.group(2)))] if k else [(nm.strip(), 1)]
    assert names == [("scale_log2", 1), ("max_dim", 1), ("fit_w", 1), ("fit_h", 1), ("flags", 1), ("crop_x", 1),
                     ("crop_y", 1), ("crop_w", 1), ("crop_h", 1), ("orient", 1), ("reserved", 6)]
    assert ctypes.sizeof(h2j.OutOpts4) == 64
    off = 0
    for (nm, n), (fn, ft) in zip(names, h2j.OutOpts4._fields_):
        assert fn == nm and getattr(h2j.OutOpts4, nm).offset == off and ctypes.sizeof(ft) == 4 * n
        off += 4 * n
    for fn, _ in h2j.OutOpts3._fields_[:9]:  # the first nine fields are h2j_out_opts3's, at its offsets
        assert getattr(h2j.OutOpts3, fn).offset == getattr(h2j.OutOpts4, fn).offset
    assert ctypes.sizeof(h2j.OutOpts3) == 48
    for sym in ("h2j_engine_transcode_multi4", "h2j_engine_submit_multi4", "h2j_engine_decode_multi4",
                "h2j_h265_to_jpeg_mem_multi4", "h2j_crop_window4", "h2j_stream_orientation"):
        assert re.search(r"\b" + sym + r"\(", src) and hasattr(h2j.load_library(), sym), sym


def test_sei_mapping_covers_the_eight_codes():
    """The model's own derivation: sixteen (flips, turns) triples, every code twice."""
    codes = sorted(O.sei_orient(h, v, k) for h in (0, 1) for v in (0, 1) for k in range(4))
    assert codes == sorted([0, 2, 3, 4, 5, 6, 7, 8] * 2)
    assert [O.sei_orient(0, 0, k) for k in range(4)] == [0, 8, 3, 6]  # anticlockwise turns
    assert O.sei_orient(1, 0, 0) == 2 and O.sei_orient(0, 1, 0) == 4


def test_crop_window4_worked_examples_and_edges():
    assert c_resolve(416, 240) == ((0, 0, 416, 240), (416, 240), 0)
    assert c_resolve(416, 240, orient=1) == c_resolve(416, 240, orient=0)  # 1 is 0
    assert c_resolve(416, 240, orient=3) == ((0, 0, 416, 240), (416, 240), 3)
    assert c_resolve(416, 240, orient=6) == ((0, 0, 240, 416), (240, 416), 6)
    assert c_resolve(416, 240, orient=8, crop=(36, 10, 200, 300), scale=1) == ((36, 10, 200, 300), (100, 150), 8)
    assert c_resolve(416, 240, orient=8, crop=(36, 10, 300, 200)) is None  # fits the decoded picture, not the oriented one
    assert c_resolve(1920, 1080, orient=6, fw=256, fh=256, flags=C.COVER) == ((0, 420, 1080, 1080), (256, 256), 6)
    assert c_resolve(416, 240, orient=5, fw=100) == ((0, 0, 240, 416), (100, 172), 5)
    for o in (-2, 9, 100, -100):
        assert c_resolve(416, 240, orient=o) is None and model(416, 240, orient=o) is None
    # auto resolves to the SEI's orientation; an explicit orientation ignores it
    assert c_resolve(416, 240, orient=-1, sei=6) == c_resolve(416, 240, orient=6)
    assert c_resolve(416, 240, orient=-1, sei=0) == c_resolve(416, 240) == c_resolve(416, 240, orient=-1, sei=1)
    assert c_resolve(416, 240, orient=2, sei=6) == ((0, 0, 416, 240), (416, 240), 2)
    assert c_resolve(416, 240, orient=-1, sei=9) is None and c_resolve(416, 240, sei=-1) is None
    # 2 x 2 pictures, and windows that touch the oriented picture's corner
    for o in range(9):
        assert c_resolve(2, 2, orient=o) == ((0, 0, 2, 2), (2, 2), 0 if o == 1 else o)
        assert c_resolve(2, 4, orient=o, crop=(0, 2, 2, 2)) == (None if o >= 5 else ((0, 2, 2, 2), (2, 2), 0 if o == 1 else o))
    assert c_resolve(72, 40, orient=7, crop=(38, 70, 2, 2)) == ((38, 70, 2, 2), (2, 2), 7)
    assert c_resolve(72, 40, orient=7, crop=(38, 70, 2, 4)) is None and c_resolve(72, 40, orient=7, crop=(40, 70, 0, 0)) is None
    assert c_resolve(72, 40, orient=4, crop=(70, 38, 0, 0)) == ((70, 38, 2, 2), (2, 2), 4)
    for k in range(6):  # every reserved word
        res = tuple(1 if i == k else 0 for i in range(6))
        assert c_resolve(416, 240, orient=6, reserved=res) is None and c_resolve(416, 240, reserved=res) is None
    assert h2j.crop_window(416, 240, orient=6, cover=(64, 64)) == ((0, 88, 240, 240), (64, 64), 6)
    assert h2j.crop_window(416, 240, orient="auto", sei_orient=8, scale=1) == ((0, 0, 240, 416), (120, 208), 8)
    assert h2j.crop_window(416, 240, cover=(64, 64)) == ((88, 0, 240, 240), (64, 64))  # no orientation: as it was
    with pytest.raises(ValueError):
        h2j.crop_window(416, 240, orient=9)


def test_crop_window4_seeded():
    rnd = random.Random(20261021)
    valid = invalid = 0
    for _ in range(5000):
        W, H = 2 * rnd.randint(1, 4096), 2 * rnd.randint(1, 4096)
        orient = rnd.choice([-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 5, 6, 7, 8, rnd.randint(-3, 10)])
        sei = rnd.choice([0, 0, 1, 2, 3, 4, 5, 6, 7, 8])
        o = O.resolve_orient(orient, sei)
        OW, OH = (H, W) if o is not None and o >= 5 else (W, H)
        pick = lambda n: rnd.choice([0, 0, 2 * rnd.randint(0, n // 2), rnd.randint(-2, n + 2)])
        crop = (pick(OW), pick(OH), pick(OW), pick(OH))
        if rnd.random() < 0.5:  # a window that certainly fits the oriented picture
            x, y = 2 * rnd.randint(0, OW // 2 - 1), 2 * rnd.randint(0, OH // 2 - 1)
            crop = (x, y, 2 * rnd.randint(1, (OW - x) // 2), 2 * rnd.randint(1, (OH - y) // 2))
        kw = dict(crop=crop, orient=orient, sei=sei)
        mode = rnd.randint(0, 4)
        if mode == 1:
            kw.update(scale=rnd.randint(-1, 4), max_dim=rnd.choice([0, 0, -1, rnd.randint(1, 2000)]))
        elif mode == 2:
            kw.update(fw=rnd.choice([0, 1, rnd.randint(2, 3000)]), fh=rnd.choice([0, rnd.randint(2, 3000)]), flags=rnd.choice([0, 0, 1, 4]))
        elif mode == 3:
            kw.update(fw=rnd.choice([0, rnd.randint(2, 3000), rnd.randint(2, 64)]), fh=rnd.choice([0, rnd.randint(2, 3000)]),
                      flags=rnd.choice([2, 2, 2, 3]))
        if rnd.random() < 0.03:
            kw["reserved"] = rnd.choice([(1, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, -1), (0, 0, 0, 5, 0, 0)])
        want, got = model(W, H, **kw), c_resolve(W, H, **kw)
        assert got == want, (W, H, kw, got, want)
        valid += want is not None
        invalid += want is None
    assert valid > 1000 and invalid > 1000, (valid, invalid)


def orientation(stream):
    return h2j.stream_orientation(stream)


@pytest.mark.parametrize("name,codec", [(HEVC, 265), (H264, 264)])
def test_stream_orientation(name, codec):
    s = read(golden(name))
    assert orientation(s) == 0  # no SEI
    for hor in (0, 1):
        for ver in (0, 1):
            for k in range(4):
                assert orientation(O.insert_sei(s, codec, hor, ver, k)) == O.sei_orient(hor, ver, k), (hor, ver, k)
    msg = lambda **kw: O.sei_message(47, O.orientation_payload(codec, **kw))
    put = lambda *messages, **kw: O.insert_nal(s, codec, O.sei_nal(codec, list(messages)), **kw)
    assert orientation(put(msg(cancel=1))) == 0
    assert orientation(put(msg(rotation=0x2000))) == 0 and orientation(put(msg(hor=1, rotation=0x4001))) == 0
    # two messages in one NAL unit, and in two: the last wins (a cancel included)
    assert orientation(put(msg(rotation=0x4000), msg(rotation=0xC000))) == 6
    two = O.insert_nal(O.insert_sei(s, codec, 0, 0, 3), codec, O.sei_nal(codec, [msg(hor=1)]))
    assert orientation(two) == 2
    assert orientation(put(msg(rotation=0x4000), msg(cancel=1))) == 0
    # an unrelated payload in front, with 00 00 01 inside (emulation prevention) and a size of 255 and more
    other = O.sei_message(5, bytes(16) + b"\x00\x00\x01\x00\x00\x00\x03" + bytes(range(40)))
    long_other = O.sei_message(300, b"\x00\x00\x02" + bytes(297))
    nal = O.sei_nal(codec, [other, long_other, msg(rotation=0x8000)])
    assert b"\x00\x00\x03" in nal[6:] and b"\x00\x00\x01" not in nal[4:]
    assert orientation(O.insert_nal(s, codec, nal)) == 3
    # a payload size that runs past the NAL unit; a payload cut short; a type with no size
    for bad in (O.sei_message(47, O.orientation_payload(codec, rotation=0x4000), size=200),
                O.sei_message(47, O.orientation_payload(codec, rotation=0x4000)[:2]),
                O.sei_message(47, b"")[:1]):
        assert orientation(O.insert_nal(s, codec, O.sei_nal(codec, [bad], trailing=False))) == 0
    # behind the first slice: not picture 0's
    assert orientation(put(msg(rotation=0x4000), after_first_slice=True)) == 0
    with pytest.raises(ValueError):
        h2j.stream_orientation(b"\x00\x00\x01\x09\x10 not a stream")


def test_spec_parsing():
    assert h2j.rendition_spec({"orient": 6}) == (0, 0, 0, 0, 0, 0, 0, 0, 0, 6)
    assert h2j.rendition_spec({"orient": "auto", "scale": 2}) == (2, 0, 0, 0, 0, 0, 0, 0, 0, -1)
    assert h2j.rendition_spec({"orient": 8, "crop": (36, 10, 200, 300), "cover": (8, 8)}) == (0, 0, 8, 8, 2, 36, 10, 200, 300, 8)
    assert h2j.rendition_spec({"orient": 0}) == (0,) * 10 and h2j.rendition_spec({"orient": 9})[9] == 9  # the engine's to judge
    for bad in ({"orient": "upright"}, {"orient": 1.5}, {"orient": True}, {"orient": None}, {"orient": (6,)}, {"orientation": 6}):
        with pytest.raises(ValueError):
            h2j.rendition_spec(bad)
    with pytest.raises(ValueError):
        h2j.normalize_renditions([0, {"orient": "left"}], 1)
    assert h2j.normalize_renditions([0, {"orient": 3}], 2) == [[(0, 0, 0, 0, 0), (0,) * 9 + (3,)]] * 2
    nrend, opts, total = h2j._multi_opts(h2j.normalize_renditions([1, {"crop": (2, 2, 8, 8)}, {"orient": "auto", "fit": (4, 0)}], 1))
    assert opts._type_ is h2j.OutOpts4 and total == 3 and list(nrend) == [3]
    assert [(o.scale_log2, o.crop_w, o.fit_w, o.orient, list(o.reserved)) for o in opts] == [
        (1, 0, 0, 0, [0] * 6), (0, 8, 0, 0, [0] * 6), (0, 0, 4, -1, [0] * 6)]
    # without an orient key: the option arrays they always were
    assert h2j._multi_opts(h2j.normalize_renditions([1, {"crop": (2, 2, 8, 8)}], 1))[1]._type_ is h2j.OutOpts3
    assert h2j._multi_opts(h2j.normalize_renditions([1, (4, 0)], 1))[1]._type_ is h2j.OutOpts2
    specs = h2j._window_specs(3, 1, None, None, False, None, None, [6, None, "auto"])
    assert [h2j.rendition_spec(s[0]) for s in specs] == [(1, 0, 0, 0, 0, 0, 0, 0, 0, 6), (1, 0, 0, 0, 0), (1, 0, 0, 0, 0, 0, 0, 0, 0, -1)]
    assert [h2j.rendition_spec(s[0])[9] for s in h2j._window_specs(2, None, None, None, False, None, None, 3)] == [3, 3]
    for bad in ([6], "left", [6, "left"]):
        with pytest.raises(ValueError):
            h2j._window_specs(2, None, None, None, False, None, None, bad)
