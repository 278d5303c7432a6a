"""Padded output without a GPU: the option struct against the header, the pure h2j_crop_window7 and h2j_pad_colour
against tests/pad_ref.py, and the Python spec parser (DESIGN.md "Padded output (K3b)")."""
import ctypes
import os
import re
import subprocess

import pytest

import h2j
import pad_ref as PAD
from conftest import PKG, ROOT
from test_rgb_api import c_window, opts6

ERR = -60
STRETCH, COVER = 1, 2


def opts7(scale=0, max_dim=0, fw=0, fh=0, flags=0, crop=(0, 0, 0, 0), orient=0, qscale=0, sharpen=0, fmt=0, pad=0, background=0, reserved=0):
    return h2j.OutOpts7(scale, max_dim, fw, fh, flags, crop[0], crop[1], crop[2], crop[3], orient, qscale, sharpen, fmt, pad, background,
                        (ctypes.c_int32 * 1)(reserved))


def window7(W, H, o, sei=0):
    win, place = (ctypes.c_int32 * 4)(7, 7, 7, 7), (ctypes.c_int32 * 4)(9, 9, 9, 9)
    ow, oh, ro = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    rc = h2j.load_library().h2j_crop_window7(W, H, ctypes.byref(o), sei, win, ctypes.byref(ow), ctypes.byref(oh), ctypes.byref(ro), place)
    if rc != 0:
        assert rc == ERR and list(win) == [7] * 4 and list(place) == [9] * 4 and (ow.value, oh.value, ro.value) == (-1, -1, -1)  # nothing written
        return None
    return tuple(win), (ow.value, oh.value), ro.value, tuple(place)


def colour(rgb):
    ycc = (ctypes.c_int * 3)(-1, -1, -1)
    rc = h2j.load_library().h2j_pad_colour(rgb, ycc)
    return tuple(ycc) if rc == 0 else rc


def test_struct_matches_header():
    src = open(os.path.join(ROOT, "include", "h2j.h")).read()
    ext = open(os.path.join(ROOT, "include", "h2j_ext.h")).read()  # the header of libH265ToJpegExt.so: the functions
    m = re.search(r"typedef struct \{([^}]*)\}\s*h2j_out_opts7;", src)
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
                     ("pad", 1), ("background", 1), ("reserved", 1)]
    assert ctypes.sizeof(h2j.OutOpts7) == ctypes.sizeof(h2j.OutOpts6) == 64
    off = 0
    for (nm, n), (fn, ft) in zip(names, h2j.OutOpts7._fields_):
        assert fn == nm and getattr(h2j.OutOpts7, nm).offset == off and ctypes.sizeof(ft) == 4 * n
        off += 4 * n
    for fn, _ in h2j.OutOpts6._fields_[:13]:  # the first thirteen fields are h2j_out_opts6's, at its offsets
        assert getattr(h2j.OutOpts6, fn).offset == getattr(h2j.OutOpts7, fn).offset
    assert h2j.OutOpts7.pad.offset == h2j.OutOpts6.reserved.offset == 52 and h2j.OutOpts7.background.offset == 56
    for sym in ("h2j_engine_transcode_multi7", "h2j_engine_submit_multi7", "h2j_h265_to_jpeg_mem_multi7", "h2j_engine_decode_multi7",
                "h2j_crop_window7", "h2j_pad_colour"):
        assert re.search(r"\b" + sym + r"\(", ext) and not re.search(r"\b" + sym + r"\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
        assert hasattr(h2j.load_library(), sym), sym
    gpu = open(os.path.join(ROOT, "include", "h2j_gpu.h")).read()
    assert re.search(r"\bint h2j_gpu_pad\(", gpu)
    assert h2j.STAT_KEYS_LATER == ["pad_bytes"] and len(h2j.STAT_KEYS) == 26


def test_the_entry_points_live_in_the_extension_library():
    """libH265ToJpeg.so's exported names are a fixed list (test_abi_exports.py); the six entry points of padded output are
    all that libH265ToJpegExt.so exports, and the binding finds them beside the others."""
    names = {}
    for lib in ("libH265ToJpeg.so", "libH265ToJpegExt.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, lib)], stdout=subprocess.PIPE, check=True).stdout.decode()
        names[lib] = sorted(f[2] for f in (l.split() for l in out.splitlines()) if len(f) == 3 and f[1] in "TW" and not f[2].startswith("_Z"))
    assert names["libH265ToJpegExt.so"] == sorted(h2j._EXT_SYMBOLS)
    assert not set(h2j._EXT_SYMBOLS) & set(names["libH265ToJpeg.so"])
    assert all(hasattr(h2j.load_library(), s) for s in h2j._EXT_SYMBOLS)


def test_pad_colour_matches_the_model():
    cols = [(r, g, b) for r in range(0, 256, 51) for g in range(0, 256, 51) for b in range(0, 256, 51)]
    cols += [(114, 114, 114), (255, 0, 16), (0, 0, 255), (1, 2, 3)] + [(v, v, v) for v in range(256)]
    for r, g, b in cols:
        assert colour((r << 16) | (g << 8) | b) == PAD.pad_colour((r, g, b)), (r, g, b)
    assert colour(1 << 24) == ERR and colour(0xFF000000) == ERR and colour(0xFFFFFF) == (255, 128, 128)
    assert h2j.load_library().h2j_pad_colour(0, None) == ERR


SIZES = [(64, 64), (72, 40), (48, 200), (416, 240), (1920, 1080), (2, 2), (240, 416)]
BOXES = [(64, 64), (70, 66), (78, 66), (90, 70), (91, 71), (50, 50), (16, 16), (6, 6), (640, 640), (224, 224), (3, 2), (2, 300), (4000, 30)]


def test_crop_window7_against_the_model():
    hits = 0
    for W, H in SIZES:
        for fw, fh in BOXES:
            for flags in (0, STRETCH, COVER):
                for orient in (0, 6):
                    crop = (0, 0, 0, 0) if W < 100 else (4, 2, W // 2, H // 2)
                    base = c_window("h2j_crop_window6", W, H, opts6(0, 0, fw, fh, flags, crop, orient, 0, 16, 1))
                    got = window7(W, H, opts7(0, 0, fw, fh, flags, crop, orient, 0, 16, 1, 1, 0x727272))
                    assert base is not None and got is not None, (W, H, fw, fh, flags)
                    win, (ow, oh), ro = base
                    bw, bh, px, py = PAD.place(ow, oh, fw, fh)
                    assert got == (win, (bw, bh), ro, (px, py, ow, oh)), (W, H, fw, fh, flags, orient, got)
                    # without pad: h2j_crop_window6's answer, the picture part all of the output
                    assert window7(W, H, opts7(0, 0, fw, fh, flags, crop, orient, 0, 16, 1)) == (win, (ow, oh), ro, (0, 0, ow, oh))
                    hits += (ow, oh) != (bw, bh)
    assert hits > 300
    # the issue's placements
    assert window7(64, 64, opts7(fw=70, fh=66, pad=1))[1:] == ((70, 66), 0, (2, 0, 64, 64))
    assert window7(64, 64, opts7(fw=100, fh=60, flags=COVER, pad=1)) == ((0, 12, 64, 38), (100, 60), 0, (18, 10, 64, 38))
    assert window7(72, 40, opts7(fw=50, fh=50, pad=1))[1:] == ((50, 50), 0, (0, 12, 50, 26))
    assert window7(48, 200, opts7(fw=16, fh=16, pad=1))[1:] == ((16, 16), 0, (6, 0, 2, 16))
    assert [window7(48, 200, opts7(fw=f, fh=100, pad=1))[3] for f in (46, 50, 54)] == [(10, 0, 24, 100), (12, 0, 24, 100), (14, 0, 24, 100)]
    assert window7(416, 240, opts7(fw=6, fh=6, pad=1))[1:] == ((6, 6), 0, (0, 2, 6, 2))
    assert window7(416, 240, opts7(fw=256, fh=256, orient=6, pad=1))[1:] == ((256, 256), 6, (54, 0, 146, 256))
    assert window7(416, 240, opts7(fw=128, fh=128, crop=(36, 10, 300, 200), pad=1)) == ((36, 10, 300, 200), (128, 128), 0, (0, 22, 128, 84))
    assert window7(320, 180, opts7(fw=400, fh=200, pad=1))[1:] == ((400, 200), 0, (40, 10, 320, 180))
    assert window7(1920, 1080, opts7(fw=640, fh=640, pad=1, background=0x727272))[1:] == ((640, 640), 0, (0, 140, 640, 360))


def test_no_border_is_the_job_without_pad():
    for W, H, fw, fh, flags in ((64, 64, 64, 64, 0), (64, 64, 65, 65, 0), (416, 240, 100, 60, STRETCH), (416, 240, 64, 64, COVER),
                                (1920, 1080, 640, 360, 0), (1920, 1080, 641, 361, 0)):
        got = window7(W, H, opts7(fw=fw, fh=fh, flags=flags, pad=1, background=0xFF0010))
        assert got == window7(W, H, opts7(fw=fw, fh=fh, flags=flags)), (W, H, fw, fh, flags)
        assert got[3] == (0, 0) + got[1]


def test_invalid_combinations():
    ok = opts7(fw=100, fh=100, pad=1, background=0x102030)
    assert window7(64, 64, ok) is not None
    bad = [opts7(fw=100, fh=100, pad=2), opts7(fw=100, fh=100, pad=-1),                      # pad outside 0..1
           opts7(fw=100, fh=100, pad=1, background=1 << 24), opts7(fw=100, fh=100, pad=1, background=-1),  # bits above 23
           opts7(fw=100, fh=100, background=1), opts7(background=0x102030),                   # a colour without pad
           opts7(pad=1), opts7(fw=100, pad=1), opts7(fh=100, pad=1), opts7(scale=1, pad=1), opts7(max_dim=64, pad=1),  # no two-sided box
           opts7(fw=8194, fh=8192, pad=1), opts7(fw=8192, fh=8194, pad=1), opts7(fw=65535, fh=65535, pad=1), opts7(fw=65534, fh=1026, pad=1),  # canvas
           opts7(fw=100, flags=STRETCH, pad=1), opts7(fw=100, fh=100, flags=STRETCH | COVER, pad=1),
           opts7(fw=100, fh=100, pad=1, reserved=1), opts7(reserved=-1), opts7(fw=100, fh=100, reserved=1 << 30)]  # reserved
    for o in bad:
        assert window7(64, 64, o) is None, [getattr(o, f) for f, _ in o._fields_[:15]]
    # valid beside them: every kind of box
    for flags in (0, STRETCH, COVER):
        assert window7(64, 64, opts7(fw=100, fh=80, flags=flags, pad=1, fmt=2, sharpen=8, orient=3)) is not None
    assert window7(64, 64, opts7(fw=100, fh=80, pad=1, qscale=5)) is not None and window7(64, 64, opts7(fw=100, fh=80, pad=1, qscale=5, fmt=1)) is None


def test_the_largest_canvas():
    """H2J_PAD_MAX_SAMPLES: the largest accepted boxes and the smallest rejected ones, whatever the picture's size; without
    pad the same boxes are what they always were."""
    src = open(os.path.join(ROOT, "include", "h2j.h")).read()
    assert re.search(r"#define H2J_PAD_MAX_SAMPLES \(1 << 26\)", src)
    for W, H in ((64, 64), (8192, 8192)):
        for fw, fh in ((8192, 8192), (8193, 8193), (65534, 1024), (65535, 1025), (1024, 65535), (2, 65535)):
            got = window7(W, H, opts7(fw=fw, fh=fh, pad=1))
            assert got is not None and got[1] == (fw & ~1, fh & ~1) and got[1][0] * got[1][1] <= 1 << 26, (W, H, fw, fh)
        for fw, fh in ((8194, 8192), (8192, 8194), (65534, 1026), (1026, 65534), (65535, 65535), (41400, 41400)):
            assert (fw & ~1) * (fh & ~1) > 1 << 26
            assert window7(W, H, opts7(fw=fw, fh=fh, pad=1)) is None and window7(W, H, opts7(fw=fw, fh=fh, flags=COVER, pad=1)) is None
            assert window7(W, H, opts7(fw=fw, fh=fh)) is not None
    # the planes' byte offsets of the largest canvases stay far inside int32
    for bw, bh in ((8192, 8192), (65534, 1024), (2, 65534)):
        stride = lambda w: (w + 15) & ~15
        assert stride(bw) * bh + 2 * stride(bw // 2) * (bh // 2) < 1 << 27


def test_opts6_items_that_carry_the_words_are_rejected():
    assert c_window("h2j_crop_window6", 64, 64, opts6(fw=100, fh=100)) is not None
    for r in ((1, 0, 0), (0, 0x727272, 0), (1, 0x727272, 0), (0, 0, 1)):
        assert c_window("h2j_crop_window6", 64, 64, opts6(fw=100, fh=100, reserved=r)) is None, r


def test_rendition_spec_shapes():
    rs = h2j.rendition_spec
    # specs without the key: the tuples they always were
    assert rs({"fit": (224, 224), "format": "rgb"}) == (0, 0, 224, 224, 0) + (0,) * 7 + (1,) and rs((100, 0)) == (0, 0, 100, 0, 0)
    assert rs({"cover": (64, 64)}) == (0, 0, 64, 64, COVER, 0, 0, 0, 0)
    # with it: the fifteen fields of h2j_out_opts7
    assert rs({"fit": (640, 640), "pad": (114, 114, 114), "format": "rgb_planar"}) == (0, 0, 640, 640, 0) + (0,) * 7 + (2, 1, 0x727272)
    assert rs({"cover": (256, 256), "pad": True}) == (0, 0, 256, 256, COVER) + (0,) * 8 + (1, 0)
    assert rs({"fit": (90, 70), "pad": [255, 0, 16], "sharpen": 16, "qscale": 3}) == (0, 0, 90, 70, 0, 0, 0, 0, 0, 0, 3, 16, 0, 1, 0xFF0010)
    assert rs({"fit": (90, 70), "pad": False}) == (0, 0, 90, 70, 0) + (0,) * 10 and rs({"pad": None, "scale": 1}) == (1,) + (0,) * 14
    assert rs({"pad": True}) == (0,) * 13 + (1, 0)  # not checked here: the engine fails it alone (no box)
    for bad in ({"pad": 1}, {"pad": (1, 2)}, {"pad": (256, 0, 0)}, {"pad": (-1, 0, 0)}, {"pad": "black"}, {"pad": (1.0, 2, 3)}, {"pad": (True, 0, 0)}):
        with pytest.raises(ValueError, match="pad"):
            rs(bad)
    with pytest.raises(ValueError, match="unknown key 'padding'"):
        rs({"padding": True})
    per = h2j.normalize_renditions([0, {"fit": (64, 64), "pad": True}, {"scale": 1, "format": "rgb"}], 2)
    nrend, o, total = h2j._multi_opts(per)
    assert o._type_ is h2j.OutOpts7 and total == 6 and list(nrend) == [3, 3]
    assert (o[1].fit_w, o[1].pad, o[1].background, list(o[1].reserved)) == (64, 1, 0, [0]) and (o[2].format, o[2].pad, o[0].pad) == (1, 0, 0)
    # specs without pad take the calls they always took
    assert h2j._multi_opts(h2j.normalize_renditions([0, {"format": "rgb"}], 1))[1]._type_ is h2j.OutOpts6
    assert h2j._multi_opts(h2j.normalize_renditions([0, {"qscale": 2}], 1))[1]._type_ is h2j.OutOpts5
    assert h2j._multi_opts(h2j.normalize_renditions([0, 1], 1))[1]._type_ is h2j.OutOpts2
    # the keyword form: one value or per-item values
    specs = h2j._window_specs(3, None, None, (224, 224), False, None, None, None, None, None, "rgb", [True, None, (1, 2, 3)])
    assert [rs(s[0])[13:] for s in specs] == [(1, 0), (), (1, 0x010203)]
    assert [rs(s[0])[13:] for s in h2j._window_specs(2, None, None, (8, 8), False, None, None, pad=(114, 114, 114))] == [(1, 0x727272)] * 2
    # a colour is a tuple or a list of three ints, as the keyword and in a spec alike
    assert [rs(s[0])[13:] for s in h2j._window_specs(3, None, None, (8, 8), False, None, None, pad=[114, 114, 114])] == [(1, 0x727272)] * 3
    assert [rs(s[0])[13:] for s in h2j._window_specs(3, None, None, (8, 8), False, None, None, pad=[True, [1, 2, 3], None])] == [(1, 0), (1, 0x010203), ()]
    with pytest.raises(ValueError, match="pad: 2 entries for 3 streams"):
        h2j._window_specs(3, None, None, (8, 8), False, None, None, pad=[True, True])
    # a padded raw rendition of a boxed spec is sized from the box
    assert h2j._multi_cap([b"x"], [[rs({"fit": (640, 640), "pad": True, "format": "rgb"})]], 1 << 20) == (1 << 20) + 3 * 640 * 640
