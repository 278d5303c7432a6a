"""RGB output without a GPU: the option struct against the header, the pure h2j_crop_window6 against
h2j_crop_window5, and the Python spec parser (DESIGN.md "RGB output (K3c)")."""
import ctypes
import os
import random
import re

import pytest

import h2j
from conftest import ROOT

ERR = -60


def c_window(fn, W, H, o, sei=0):
    win, ow, oh, ro = (ctypes.c_int32 * 4)(7, 7, 7, 7), ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    rc = getattr(h2j.load_library(), fn)(W, H, ctypes.byref(o), sei, win, ctypes.byref(ow), ctypes.byref(oh), ctypes.byref(ro))
    if rc != 0:
        assert rc == ERR and list(win) == [7, 7, 7, 7] and (ow.value, oh.value, ro.value) == (-1, -1, -1)  # nothing written
        return None
    return tuple(win), (ow.value, oh.value), ro.value


def opts6(scale=0, max_dim=0, fw=0, fh=0, flags=0, crop=(0, 0, 0, 0), orient=0, qscale=0, sharpen=0, fmt=0, reserved=(0,) * 3):
    return h2j.OutOpts6(scale, max_dim, fw, fh, flags, crop[0], crop[1], crop[2], crop[3], orient, qscale, sharpen, fmt,
                        (ctypes.c_int32 * 3)(*reserved))


def opts5(scale=0, max_dim=0, fw=0, fh=0, flags=0, crop=(0, 0, 0, 0), orient=0, qscale=0, sharpen=0, reserved=(0,) * 4):
    return h2j.OutOpts5(scale, max_dim, fw, fh, flags, crop[0], crop[1], crop[2], crop[3], orient, qscale, sharpen,
                        (ctypes.c_int32 * 4)(*reserved))


def test_struct_matches_header():
    src = open(os.path.join(ROOT, "include", "h2j.h")).read()
    m = re.search(r"typedef struct \{([^}]*)\}\s*h2j_out_opts6;", src)
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
                     ("crop_y", 1), ("crop_w", 1), ("crop_h", 1), ("orient", 1), ("qscale", 1), ("sharpen", 1), ("format", 1),
                     ("reserved", 3)]
    assert ctypes.sizeof(h2j.OutOpts6) == ctypes.sizeof(h2j.OutOpts5) == 64
    off = 0
    for (nm, n), (fn, ft) in zip(names, h2j.OutOpts6._fields_):
        assert fn == nm and getattr(h2j.OutOpts6, nm).offset == off and ctypes.sizeof(ft) == 4 * n
        off += 4 * n
    for fn, _ in h2j.OutOpts5._fields_[:12]:  # the first twelve fields are h2j_out_opts5's, at its offsets
        assert getattr(h2j.OutOpts5, fn).offset == getattr(h2j.OutOpts6, fn).offset
    assert h2j.OutOpts6.format.offset == h2j.OutOpts5.reserved.offset == 48  # the new field: its first reserved word
    for name, val in (("H2J_FMT_JPEG", 0), ("H2J_FMT_RGB8", 1), ("H2J_FMT_RGB8_PLANAR", 2)):
        assert re.search(r"#define " + name + r" " + str(val) + r"\b", src), name
    assert (h2j.FMT_JPEG, h2j.FMT_RGB8, h2j.FMT_RGB8_PLANAR) == (0, 1, 2)
    assert h2j.FORMATS == {"jpeg": 0, "rgb": 1, "rgb_planar": 2}
    for sym in ("h2j_engine_transcode_multi6", "h2j_engine_submit_multi6", "h2j_h265_to_jpeg_mem_multi6", "h2j_crop_window6"):
        assert re.search(r"\b" + sym + r"\(", src) and hasattr(h2j.load_library(), sym), sym
    gpu = open(os.path.join(ROOT, "include", "h2j_gpu.h")).read()
    assert re.search(r"\bint h2j_gpu_rgb\(", gpu)
    assert h2j.STAT_KEYS[-1] == "raw_bytes" and h2j.STAT_KEYS[23:25] == ["renditions", "parsed"] and len(h2j.STAT_KEYS) == 26


def test_crop_window6_formats():
    for fmt in range(-2, 6):
        assert (c_window("h2j_crop_window6", 416, 240, opts6(fmt=fmt)) is not None) == (0 <= fmt <= 2), fmt
    assert c_window("h2j_crop_window6", 416, 240, opts6(fmt=3)) is None and c_window("h2j_crop_window6", 416, 240, opts6(fmt=-1)) is None
    # a raw format together with a quantiser scale: there is no quantiser
    for fmt in (1, 2):
        assert c_window("h2j_crop_window6", 416, 240, opts6(fmt=fmt, qscale=5)) is None
        assert c_window("h2j_crop_window6", 416, 240, opts6(fmt=fmt, sharpen=16)) == ((0, 0, 416, 240), (416, 240), 0)
    assert c_window("h2j_crop_window6", 416, 240, opts6(fmt=0, qscale=5)) == ((0, 0, 416, 240), (416, 240), 0)
    assert c_window("h2j_crop_window6", 416, 240, opts6(fmt=1, orient=6, scale=1, sharpen=64)) == ((0, 0, 240, 416), (120, 208), 6)
    assert c_window("h2j_crop_window6", 1920, 1080, opts6(fmt=2, fw=224, fh=224)) == ((0, 0, 1920, 1080), (224, 126), 0)
    for k in range(3):
        for val in (1, -1, 1 << 30):
            r = [0] * 3
            r[k] = val
            assert c_window("h2j_crop_window6", 416, 240, opts6(reserved=r)) is None
            assert c_window("h2j_crop_window6", 416, 240, opts6(fmt=1, reserved=r)) is None
    # the multi5 form keeps rejecting every non-zero reserved word, the one that became a field included
    for k in range(4):
        for val in (1, 2, 3, -1):
            r = [0] * 4
            r[k] = val
            assert c_window("h2j_crop_window5", 416, 240, opts5(reserved=r)) is None, (k, val)


def test_crop_window6_is_crop_window5_without_the_format():
    rng = random.Random(6)
    hits = 0
    for _ in range(400):
        W, H = 2 * rng.randint(1, 300), 2 * rng.randint(1, 300)
        kind = rng.randint(0, 3)
        scale, max_dim, fw, fh, flags = 0, 0, 0, 0, 0
        if kind == 1:
            scale, max_dim = rng.randint(0, 4), rng.choice([0, 0, 50, 200])
        elif kind == 2:
            fw, fh, flags = rng.choice([0, 1, 30, 100, 700]), rng.choice([0, 30, 100, 700]), rng.choice([0, 0, 1, 2, 3])
        crop = rng.choice([(0, 0, 0, 0), (2 * rng.randint(0, 40), 2 * rng.randint(0, 40), 2 * rng.randint(0, 150), 2 * rng.randint(0, 150)),
                           (1, 0, 0, 0)])
        orient, sei, a = rng.randint(-2, 9), rng.randint(0, 8), rng.choice([0, 0, 16, 65])
        base = c_window("h2j_crop_window5", W, H, opts5(scale, max_dim, fw, fh, flags, crop, orient, 0, a), sei)
        for fmt in (0, 1, 2):  # the format changes neither the window nor the size
            assert c_window("h2j_crop_window6", W, H, opts6(scale, max_dim, fw, fh, flags, crop, orient, 0, a, fmt), sei) == base
        hits += base is not None
    assert 50 < hits < 350


def test_rendition_spec_shapes():
    rs = h2j.rendition_spec
    # specs without the key: the tuples they always were
    assert rs(1) == (1, 0, 0, 0, 0) and rs((100, 0)) == (0, 0, 100, 0, 0) and rs({"scale": 2}) == (2, 0, 0, 0, 0)
    assert rs({"crop": (2, 4, 6, 8)}) == (0, 0, 0, 0, 0, 2, 4, 6, 8) and rs({"orient": 6}) == (0,) * 9 + (6,)
    assert rs({"qscale": 5}) == (0,) * 10 + (5, 0) and rs({"sharpen": 16, "scale": 2}) == (2,) + (0,) * 10 + (16,)
    # with it: the thirteen fields of h2j_out_opts6
    assert rs({"format": "rgb"}) == (0,) * 12 + (1,)
    assert rs({"fit": (224, 224), "format": "rgb"}) == (0, 0, 224, 224, 0) + (0,) * 7 + (1,)
    assert rs({"format": "rgb_planar", "scale": 3}) == (3,) + (0,) * 11 + (2,)
    assert rs({"format": "jpeg", "qscale": 4}) == (0,) * 10 + (4, 0, 0)
    assert rs({"format": None, "orient": 6}) == (0,) * 9 + (6, 0, 0, 0)
    assert rs({"format": "rgb", "sharpen": 16, "orient": 6, "cover": (64, 64)}) == (0, 0, 64, 64, h2j.FIT_COVER, 0, 0, 0, 0, 6, 0, 16, 1)
    assert rs({"format": "rgb", "qscale": 5}) == (0,) * 10 + (5, 0, 1)  # not checked here: the engine fails it alone
    for bad in ({"format": "bgr"}, {"format": 1}, {"format": "RGB"}, {"format": ("rgb",)}, {"format": True}):
        with pytest.raises(ValueError, match="format"):
            rs(bad)
    with pytest.raises(ValueError, match="unknown key 'fmt'"):
        rs({"fmt": "rgb"})
    with pytest.raises(ValueError, match="format 'yuv'"):
        h2j.normalize_renditions([0, {"format": "yuv"}], 2)
    per = h2j.normalize_renditions([0, {"scale": 3}, {"scale": 3, "format": "rgb"}, {"scale": 1, "format": "rgb_planar"}], 2)
    assert per == [[(0, 0, 0, 0, 0), (3, 0, 0, 0, 0), (3,) + (0,) * 11 + (1,), (1,) + (0,) * 11 + (2,)]] * 2
    # the multi6 struct only when a rendition names a format
    nrend, o, total = h2j._multi_opts(per)
    assert o._type_ is h2j.OutOpts6 and total == 8 and list(nrend) == [4, 4]
    assert (o[2].scale_log2, o[2].format, list(o[2].reserved)) == (3, 1, [0, 0, 0]) and (o[3].format, o[0].format) == (2, 0)
    assert h2j._multi_opts(h2j.normalize_renditions([0, {"qscale": 2}], 1))[1]._type_ is h2j.OutOpts5
    assert h2j._multi_opts(h2j.normalize_renditions([0, {"orient": 6}], 1))[1]._type_ is h2j.OutOpts4
    assert h2j._multi_opts(h2j.normalize_renditions([0, {"crop": (0, 0, 8, 8)}], 1))[1]._type_ is h2j.OutOpts3
    assert h2j._multi_opts(h2j.normalize_renditions([0, 1], 1))[1]._type_ is h2j.OutOpts2
    # the keyword form: one name or per-item names
    specs = h2j._window_specs(3, [1, 0, 0], None, (224, 224), False, None, None, None, None, None, ["rgb", None, "rgb_planar"])
    assert [rs(s[0])[12:] for s in specs] == [(1,), (), (2,)]
    assert [rs(s[0])[12] for s in h2j._window_specs(2, None, None, None, False, None, None, None, None, None, "rgb")] == [1, 1]
    with pytest.raises(ValueError, match="format: 2 entries for 3 streams"):
        h2j._window_specs(3, None, None, None, False, None, None, None, None, None, ["rgb", "rgb"])
