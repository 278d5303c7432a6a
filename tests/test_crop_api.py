"""Crop and cover without a GPU: the window and cover rule (the C library's pure h2j_crop_window against
tests/crop_ref.py), the struct and constants against the header, the Python spec parser, and plan_chunk on
a frame with two windows (a small host program built from chunk_plan.cpp)."""
import ctypes
import os
import random
import re
import subprocess

import pytest

import crop_ref as C
import h2j
from conftest import PKG, ROOT

ERR = -60


def c_resolve(W, H, scale=0, max_dim=0, fw=0, fh=0, flags=0, crop=(0, 0, 0, 0), reserved=(0, 0, 0)):
    lib = h2j.load_library()
    o = h2j.OutOpts3(scale, max_dim, fw, fh, flags, crop[0], crop[1], crop[2], crop[3], (ctypes.c_int32 * 3)(*reserved))
    win, ow, oh = (ctypes.c_int32 * 4)(7, 7, 7, 7), ctypes.c_int(-1), ctypes.c_int(-1)
    rc = lib.h2j_crop_window(W, H, ctypes.byref(o), win, ctypes.byref(ow), ctypes.byref(oh))
    if rc != 0:
        assert rc == ERR and list(win) == [7, 7, 7, 7] and (ow.value, oh.value) == (-1, -1)  # nothing written
        return None
    return tuple(win), (ow.value, oh.value)


def test_worked_examples():
    assert c_resolve(1920, 1080, fw=256, fh=256, flags=C.COVER) == ((420, 0, 1080, 1080), (256, 256))
    assert c_resolve(1920, 1080, fw=540, fh=540, flags=C.COVER) == ((420, 0, 1080, 1080), (540, 540))
    assert c_resolve(1920, 1080, fw=640, fh=360, flags=C.COVER) == ((0, 0, 1920, 1080), (640, 360))
    assert c_resolve(48, 200, fw=16, fh=16, flags=C.COVER) == ((0, 76, 48, 48), (16, 16))
    assert C.resolve(1920, 1080, fw=540, fh=540, flags=C.COVER)[2] == 1  # exactly 1/2: K3s
    assert C.resolve(1920, 1080, fw=256, fh=256, flags=C.COVER)[2] == C.RESAMPLE
    assert c_resolve(416, 240) == ((0, 0, 416, 240), (416, 240))
    assert c_resolve(416, 240, crop=(36, 10, 0, 0), scale=2) == ((36, 10, 380, 230), (96, 58))
    assert h2j.crop_window(1920, 1080, cover=(256, 256)) == ((420, 0, 1080, 1080), (256, 256))
    assert h2j.crop_window(416, 240, crop=(36, 10, 300, 200), fit=(100, 0)) == ((36, 10, 300, 200), (100, 66))
    with pytest.raises(ValueError):
        h2j.crop_window(416, 240, crop=(36, 10, 400, 200))


def test_cover_all_small_sizes():
    """Every even W, H in 2..40 crossed with every box bw, bh in 2..44 (739,600 cases): the C function
    against the model, and the properties the rule promises."""
    fn = h2j.load_library().h2j_crop_window
    o = h2j.OutOpts3(flags=C.COVER)
    win, ow, oh = (ctypes.c_int32 * 4)(), ctypes.c_int(0), ctypes.c_int(0)
    po, pw, ph = ctypes.byref(o), ctypes.byref(ow), ctypes.byref(oh)
    n = 0
    for W in range(2, 41, 2):
        for H in range(2, 41, 2):
            for bw in range(2, 45):
                o.fit_w = bw
                for bh in range(2, 45):
                    o.fit_h = bh
                    assert fn(W, H, po, win, pw, ph) == 0, (W, H, bw, bh)
                    got = ((win[0], win[1], win[2], win[3]), (ow.value, oh.value))
                    want = C.resolve(W, H, fw=bw, fh=bh, flags=C.COVER)
                    assert want is not None and got == want[:2], (W, H, bw, bh, got, want)
                    (x, y, w, h), (a, b) = got
                    assert (x | y | w | h | a | b) & 1 == 0
                    assert 2 <= w <= W and 2 <= h <= H and x + w <= W and y + h <= H and 2 <= a <= w and 2 <= b <= h
                    n += 1
    assert n == 20 * 20 * 43 * 43


def test_seeded_windows_and_options():
    rnd = random.Random(20261020)
    valid = invalid = 0
    for _ in range(6000):
        W, H = 2 * rnd.randint(1, 4096), 2 * rnd.randint(1, 4096)
        pick = lambda n: rnd.choice([0, 0, 2 * rnd.randint(0, n // 2), rnd.randint(-2, n + 2)])
        crop = (pick(W), pick(H), pick(W), pick(H))
        if rnd.random() < 0.5:  # a window that certainly fits
            x, y = 2 * rnd.randint(0, W // 2 - 1), 2 * rnd.randint(0, H // 2 - 1)
            crop = (x, y, 2 * rnd.randint(1, (W - x) // 2), 2 * rnd.randint(1, (H - y) // 2))
        kw = dict(crop=crop)
        mode = rnd.randint(0, 5)
        if mode == 1:
            kw.update(scale=rnd.randint(-1, 4), max_dim=rnd.choice([0, 0, -1, rnd.randint(1, 2000)]))
        elif mode == 2:
            kw.update(fw=rnd.choice([0, 1, rnd.randint(2, 3000)]), fh=rnd.choice([0, rnd.randint(2, 3000)]),
                      flags=rnd.choice([0, 0, 1, 4]))
        elif mode >= 3:
            kw.update(fw=rnd.choice([0, 1, rnd.randint(2, 3000), rnd.randint(2, 64)]), fh=rnd.choice([0, rnd.randint(2, 3000)]),
                      flags=rnd.choice([2, 2, 2, 3, 6]), scale=rnd.choice([0, 0, 0, 1]), max_dim=rnd.choice([0, 0, 0, 100]))
        if rnd.random() < 0.03:
            kw["reserved"] = rnd.choice([(1, 0, 0), (0, 0, -1)])
        want = C.resolve(W, H, **kw)
        got = c_resolve(W, H, **kw)
        assert got == (None if want is None else want[:2]), (W, H, kw, got, want)
        valid += want is not None
        invalid += want is None
    assert valid > 1000 and invalid > 1000, (valid, invalid)
    for W, H in ((3, 4), (4, 0), (65538, 4)):  # not a picture size
        assert c_resolve(W, H) is None and C.resolve(W, H) is None


def test_struct_and_constants_match_header():
    src = open(os.path.join(ROOT, "include", "h2j.h")).read()
    m = re.search(r"#define\s+H2J_FIT_COVER\s+(\d+)", src)
    assert m and int(m.group(1)) == h2j.FIT_COVER == C.COVER
    m = re.search(r"typedef struct \{([^}]*)\}\s*h2j_out_opts3;", src)
    assert m
    names = []
    for decl in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        assert decl.startswith("int32_t "), decl
        for nm in decl[len("int32_t "):].split(","):
            nm = nm.strip()
            k = re.match(r"(\w+)\[(\d+)\]$", nm)
            names += [(k.group(1), int(k.group(2)))] if k else [(nm, 1)]
    assert names == [("scale_log2", 1), ("max_dim", 1), ("fit_w", 1), ("fit_h", 1), ("flags", 1), ("crop_x", 1),
                     ("crop_y", 1), ("crop_w", 1), ("crop_h", 1), ("reserved", 3)]
    assert ctypes.sizeof(h2j.OutOpts3) == 48
    off = 0
    for (nm, n), (fn, ft) in zip(names, h2j.OutOpts3._fields_):
        assert fn == nm and getattr(h2j.OutOpts3, nm).offset == off and ctypes.sizeof(ft) == 4 * n
        off += 4 * n
    # the first five fields are h2j_out_opts2's, at its offsets
    for fn, _ in h2j.OutOpts2._fields_[:5]:
        assert getattr(h2j.OutOpts2, fn).offset == getattr(h2j.OutOpts3, fn).offset
    assert ctypes.sizeof(h2j.OutOpts2) == 32
    for sym in ("h2j_engine_transcode_multi3", "h2j_engine_submit_multi3", "h2j_engine_decode_multi3",
                "h2j_h265_to_jpeg_mem_multi3", "h2j_crop_window"):
        assert re.search(r"\b" + sym + r"\(", src) and hasattr(h2j.load_library(), sym), sym


def test_spec_parsing():
    assert h2j.rendition_spec({"crop": (2, 4, 60, 30)}) == (0, 0, 0, 0, 0, 2, 4, 60, 30)
    assert h2j.rendition_spec({"crop": (2, 4, 0, None), "scale": 2}) == (2, 0, 0, 0, 0, 2, 4, 0, 0)
    assert h2j.rendition_spec({"cover": (256, 256)}) == (0, 0, 256, 256, h2j.FIT_COVER, 0, 0, 0, 0)
    assert h2j.rendition_spec({"cover": (16, 0), "crop": [0, 0, 32, 32], "stretch": True}) == (0, 0, 16, 0, 3, 0, 0, 32, 32)
    assert h2j.rendition_spec({"crop": (-2, 1, 3, 5), "fit": (10, 0)}) == (0, 0, 10, 0, 0, -2, 1, 3, 5)  # the engine's to judge
    for bad in ({"crop": (1, 2, 3)}, {"crop": 4}, {"crop": (0, 0, 1.5, 2)}, {"crop": "0,0,2,2"}, {"cover": 16},
                {"cover": (1, 2, 3)}, {"cover": (16, 16), "fit": (16, 16)}, {"crop": (0, 0, True, 2)}, {"window": (0, 0, 2, 2)}):
        with pytest.raises(ValueError):
            h2j.rendition_spec(bad)
    # old specs give the old tuples, and old option arrays
    assert h2j.rendition_spec({"fit": (62, 38), "stretch": True}) == (0, 0, 62, 38, h2j.FIT_STRETCH)
    assert h2j.rendition_spec(3) == (3, 0, 0, 0, 0) and h2j.rendition_spec((50, 0)) == (0, 0, 50, 0, 0)
    assert h2j.normalize_renditions([0, {"cover": (8, 8)}], 2) == [[(0, 0, 0, 0, 0), (0, 0, 8, 8, 2, 0, 0, 0, 0)]] * 2
    _, opts, total = h2j._multi_opts(h2j.normalize_renditions([0, (50, 0)], 1))
    assert opts._type_ is h2j.OutOpts2 and total == 2
    nrend, opts, total = h2j._multi_opts(h2j.normalize_renditions([1, {"crop": (2, 2, 8, 8), "fit": (4, 0)}], 1))
    assert opts._type_ is h2j.OutOpts3 and total == 2 and list(nrend) == [2]
    assert (opts[0].scale_log2, opts[0].crop_w, opts[1].fit_w, opts[1].crop_x, opts[1].crop_w) == (1, 0, 4, 2, 8)
    assert h2j._out_opts(1, None, 2)._type_ is h2j.OutOpts and h2j._out_opts(None, None, 2) is None
    specs = h2j._window_specs(2, 1, None, None, False, (2, 2, 8, 8), [None, (4, 4)])
    assert [h2j.rendition_spec(s[0]) for s in specs] == [(1, 0, 0, 0, 0, 2, 2, 8, 8), (1, 0, 4, 4, 2, 2, 2, 8, 8)]
    with pytest.raises(ValueError):
        h2j._window_specs(2, None, None, None, False, [(0, 0, 2, 2)], None)  # one window for two streams
    with pytest.raises(ValueError):
        h2j._window_specs(1, None, None, None, False, [(0, 0, 2)], None)


def test_plan_chunk_windows(tmp_path):
    """Window A at scales 1, 2, 3, window B at scale 1 and the whole picture: one pyramid for A, one K3s entry
    for B, five views with the unscaled whole picture first; a lone unscaled 16-aligned window of a picture
    with SAO is summed by K4a into a jstat that K3 SAO does not write."""
    exe = str(tmp_path / "plan_chunk_case")
    host = os.path.join(PKG, "csrc", "host")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++11", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + host, "-o", exe,
                           os.path.join(ROOT, "tests", "plan_chunk", "plan_chunk_case.cpp"), os.path.join(host, "chunk_plan.cpp")])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    lines = out.stdout.decode().splitlines()
    get = lambda key: [l.split()[1:] for l in lines if l.split()[0] == key]
    assert get("nf") == [["2", "nv", "6", "njstat", "7", "wins", "3", "views", "1"]]
    # frame 0: the unscaled whole picture first, then A's levels and B's; frame 1: its window
    assert [" ".join(v) for v in get("view")] == [
        "0 frame 0 src 0 scale 0 size 416 240", "1 frame 0 src 2 scale 1 size 150 100", "2 frame 0 src 2 scale 2 size 76 50",
        "3 frame 0 src 2 scale 3 size 38 26", "4 frame 0 src 3 scale 1 size 22 18", "5 frame 1 src 4 scale 0 size 64 48"]
    assert [" ".join(v) for v in get("rend")] == ["0 view 1", "1 view 2", "2 view 3", "3 view 4", "4 view 0", "5 view 5"]
    assert [" ".join(v) for v in get("pyramid")] == ["frame 2 mask 14 sizes 150 76 38"]
    assert [" ".join(v) for v in get("k3s")] == ["frame 3 scale 1 size 22 18"]
    assert [" ".join(v) for v in get("wframe")] == ["0 crop 36 10 out 300 200 pic2 1", "1 crop 2 6 out 44 36 pic2 1",
                                                    "2 crop 16 16 out 64 48 pic2 1"]
    assert get("window_view") == [["crop", "16", "16", "out", "64", "48", "pic_is_pic2", "1", "own_jstat", "1",
                                   "frame_folds", "1", "view_folds", "0"]]
    # frame 0 keeps its first view's jstat; frame 1 has slot 6, behind the views'; K4a sums all but view 0
    assert get("fstat") == [["0", "6", "k4a_frames", "5", "staging_frames", "5"]]
