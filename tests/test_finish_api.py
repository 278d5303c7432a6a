"""Finishing (qscale, sharpen) without a GPU: the option struct against the header, the pure h2j_crop_window5
against h2j_crop_window4, the Python spec parser, and what the host engine hands to the kernel library -- against
the host-memory stand-in without the stage (tests/fake_gpu/fake_gpu.cpp) and one with it
(tests/fake_gpu/fake_gpu_finish.cpp), built and selected as test_orient_handover.py does it."""
import ctypes
import json
import os
import random
import re
import shutil
import subprocess
import sys

import pytest

import finish_handover_cases as FC
import h2j
import handover_cases as H
from conftest import PKG, ROOT
from test_orient_handover import assert_same, sections_of

ERR, ERR_NO_STAGE = -60, -62


def c_window(fn, W, H, o, sei=0):
    win, ow, oh, ro = (ctypes.c_int32 * 4)(7, 7, 7, 7), ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    rc = getattr(h2j.load_library(), fn)(W, H, ctypes.byref(o), sei, win, ctypes.byref(ow), ctypes.byref(oh), ctypes.byref(ro))
    if rc != 0:
        assert rc == ERR and list(win) == [7, 7, 7, 7] and (ow.value, oh.value, ro.value) == (-1, -1, -1)  # nothing written
        return None
    return tuple(win), (ow.value, oh.value), ro.value


def opts5(scale=0, max_dim=0, fw=0, fh=0, flags=0, crop=(0, 0, 0, 0), orient=0, qscale=0, sharpen=0, reserved=(0,) * 4):
    return h2j.OutOpts5(scale, max_dim, fw, fh, flags, crop[0], crop[1], crop[2], crop[3], orient, qscale, sharpen,
                        (ctypes.c_int32 * 4)(*reserved))


def test_struct_matches_header():
    src = open(os.path.join(ROOT, "include", "h2j.h")).read()
    m = re.search(r"typedef struct \{([^}]*)\}\s*h2j_out_opts5;", src)
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
                     ("crop_y", 1), ("crop_w", 1), ("crop_h", 1), ("orient", 1), ("qscale", 1), ("sharpen", 1), ("reserved", 4)]
    assert ctypes.sizeof(h2j.OutOpts5) == ctypes.sizeof(h2j.OutOpts4) == 64
    off = 0
    for (nm, n), (fn, ft) in zip(names, h2j.OutOpts5._fields_):
        assert fn == nm and getattr(h2j.OutOpts5, nm).offset == off and ctypes.sizeof(ft) == 4 * n
        off += 4 * n
    for fn, _ in h2j.OutOpts4._fields_[:10]:  # the first ten fields are h2j_out_opts4's, at its offsets
        assert getattr(h2j.OutOpts4, fn).offset == getattr(h2j.OutOpts5, fn).offset
    # the two new fields are the first two reserved words of h2j_out_opts4
    assert h2j.OutOpts5.qscale.offset == h2j.OutOpts4.reserved.offset == 40 and h2j.OutOpts5.sharpen.offset == 44
    for sym in ("h2j_engine_transcode_multi5", "h2j_engine_submit_multi5", "h2j_engine_decode_multi5",
                "h2j_h265_to_jpeg_mem_multi5", "h2j_crop_window5"):
        assert re.search(r"\b" + sym + r"\(", src) and hasattr(h2j.load_library(), sym), sym


def test_crop_window5_ranges():
    for q in range(-1, 34):
        ok = q == 0 or 2 <= q <= 31
        assert (c_window("h2j_crop_window5", 416, 240, opts5(qscale=q)) is not None) == ok, q
    for a in range(-1, 67):
        assert (c_window("h2j_crop_window5", 416, 240, opts5(sharpen=a)) is not None) == (0 <= a <= 64), a
    assert c_window("h2j_crop_window5", 416, 240, opts5(qscale=31, sharpen=64, orient=6, scale=1)) == ((0, 0, 240, 416), (120, 208), 6)
    for k in range(4):
        for val in (1, -1, 1 << 30):
            r = [0] * 4
            r[k] = val
            assert c_window("h2j_crop_window5", 416, 240, opts5(reserved=r)) is None
            assert c_window("h2j_crop_window5", 416, 240, opts5(qscale=5, sharpen=5, reserved=r)) is None
    # the multi4 form keeps rejecting every non-zero reserved word, the two that became fields included
    for k in range(6):
        r = [0] * 6
        r[k] = 5
        o4 = h2j.OutOpts4(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, (ctypes.c_int32 * 6)(*r))
        assert c_window("h2j_crop_window4", 416, 240, o4) is None, k


def test_crop_window5_is_crop_window4_without_the_options():
    rng = random.Random(5)
    hits = 0
    for _ in range(600):
        W, H = 2 * rng.randint(1, 300), 2 * rng.randint(1, 300)
        kind = rng.randint(0, 3)
        scale, max_dim, fw, fh, flags = 0, 0, 0, 0, 0
        if kind == 1:
            scale, max_dim = rng.randint(0, 4), rng.choice([0, 0, 50, 200])
        elif kind == 2:
            fw, fh, flags = rng.choice([0, 1, 30, 100, 700]), rng.choice([0, 30, 100, 700]), rng.choice([0, 0, 1, 2, 3])
        crop = rng.choice([(0, 0, 0, 0), (2 * rng.randint(0, 40), 2 * rng.randint(0, 40), 2 * rng.randint(0, 150), 2 * rng.randint(0, 150)),
                           (1, 0, 0, 0)])
        orient, sei = rng.randint(-2, 9), rng.randint(0, 8)
        o4 = h2j.OutOpts4(scale, max_dim, fw, fh, flags, crop[0], crop[1], crop[2], crop[3], orient, (ctypes.c_int32 * 6)())
        a = c_window("h2j_crop_window4", W, H, o4, sei)
        b = c_window("h2j_crop_window5", W, H, opts5(scale, max_dim, fw, fh, flags, crop, orient), sei)
        assert a == b, (W, H, scale, max_dim, fw, fh, flags, crop, orient, sei)
        # ... and the options change neither the window nor the size
        assert c_window("h2j_crop_window5", W, H, opts5(scale, max_dim, fw, fh, flags, crop, orient, qscale=9, sharpen=33), sei) == a
        hits += a is not None
    assert 100 < hits < 500


def test_rendition_spec_shapes():
    rs = h2j.rendition_spec
    assert rs({"qscale": 5}) == (0,) * 10 + (5, 0)
    assert rs({"sharpen": 16, "scale": 2}) == (2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 16)
    assert rs({"qscale": 3, "sharpen": 7, "orient": 6, "crop": (2, 4, 6, 8)}) == (0, 0, 0, 0, 0, 2, 4, 6, 8, 6, 3, 7)
    assert rs({"qscale": 31, "cover": (64, 64)}) == (0, 0, 64, 64, h2j.FIT_COVER, 0, 0, 0, 0, 0, 31, 0)
    assert rs({"qscale": 0}) == (0,) * 12 and rs({"sharpen": None, "fit": (100, 0)}) == (0, 0, 100, 0, 0) + (0,) * 7
    assert rs({"orient": 6}) == (0,) * 9 + (6,) and rs(1) == (1, 0, 0, 0, 0)  # without the keys: what they were
    assert rs({"qscale": 99}) == (0,) * 10 + (99, 0)  # not range-checked here: the engine fails it alone
    for bad in ({"qscale": "5"}, {"sharpen": 1.5}, {"qscale": True}, {"sharpen": (1, 2)}):
        with pytest.raises(ValueError):
            rs(bad)
    with pytest.raises(ValueError, match="unknown key 'quality'"):
        rs({"quality": 80})
    with pytest.raises(ValueError, match="unknown key 'sharp'"):
        rs({"sharp": 1, "qscale": 2})
    per = h2j.normalize_renditions([0, {"qscale": 2}, (100, 0), {"scale": 2, "qscale": 5, "sharpen": 16}], 2)
    assert per == [[(0, 0, 0, 0, 0), (0,) * 10 + (2, 0), (0, 0, 100, 0, 0), (2,) + (0,) * 9 + (5, 16)]] * 2
    # the multi5 struct only when a rendition names one of the keys
    assert h2j._multi_opts(per)[1]._type_ is h2j.OutOpts5
    assert h2j._multi_opts(h2j.normalize_renditions([0, {"orient": 6}], 1))[1]._type_ is h2j.OutOpts4
    assert h2j._multi_opts(h2j.normalize_renditions([0, {"crop": (0, 0, 8, 8)}], 1))[1]._type_ is h2j.OutOpts3
    assert h2j._multi_opts(h2j.normalize_renditions([0, 1], 1))[1]._type_ is h2j.OutOpts2
    o = h2j._multi_opts(per)[1]
    assert (o[3].scale_log2, o[3].qscale, o[3].sharpen, list(o[3].reserved)) == (2, 5, 16, [0, 0, 0, 0]) and o[1].qscale == 2
    # the keyword form: scalars or per-item values
    specs = h2j._window_specs(3, [1, 0, 0], None, None, False, None, None, None, [5, None, 3], 16)
    assert [rs(s[0])[10:] for s in specs] == [(5, 16), (0, 16), (3, 16)]
    with pytest.raises(ValueError, match="qscale: 2 entries for 3 streams"):
        h2j._window_specs(3, None, None, None, False, None, None, None, [5, 3], None)


# ---- hand-over

IDENT = "fake_gpu: host-memory stand-in for libh2j_hip.so"


def build_fake(tmp_path_factory, name, source):
    host = os.path.join(PKG, "libH265ToJpeg.so")
    assert os.path.exists(host), f"{host} is not built: run __graft_entry__.build() first"
    d = str(tmp_path_factory.mktemp(name))
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-shared", "-fPIC", "-Wall",
                           "-I" + os.path.join(ROOT, "include"), "-o", os.path.join(d, "libh2j_hip.so"),
                           os.path.join(ROOT, "tests", "fake_gpu", source)])
    shutil.copy(host, d)
    return d


@pytest.fixture(scope="module")
def old_dir(tmp_path_factory):
    return build_fake(tmp_path_factory, "fake_gpu_old", "fake_gpu.cpp")


@pytest.fixture(scope="module")
def new_dir(tmp_path_factory):
    return build_fake(tmp_path_factory, "fake_gpu_finish", "fake_gpu_finish.cpp")


_runs = {}


def run_case(lib_dir, case):
    if case not in _runs:
        env = dict(os.environ, H2J_LIB_DIR=lib_dir)
        for k in ("H2J_CHUNK", "H2J_ENGINES", "H2J_STRICT_REFERENCE", "H2J_TAIL", "H2J_TAIL_MIN"):
            env.pop(k, None)
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "finish_handover_cases.py"), case], env=env,
                           stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=120)
        text = p.stderr.decode()
        assert p.returncode == 0, text[-2000:]
        assert text.split("\n", 1)[0] == IDENT, text[:500]
        _runs[case] = (text, [json.loads(l[7:]) for l in text.splitlines() if l.startswith("result ")])
    return _runs[case]


def test_finishing_rendition_fails_alone_without_the_stage(old_dir):
    with_, without, dec = run_case(old_dir, "a")[1]
    o, w, kept_items = 0, 0, 0  # output indices with / without the finishing renditions
    for i, (idx, specs) in enumerate(FC.ITEMS_A):
        size = H.POOL[idx][1]
        kept = FC.without_finished(specs)
        q2 = 0
        for q, spec in enumerate(specs):
            st, sof, msg = with_["status"][i][q], with_["sof"][i][q], with_["errors"][o]
            o += 1
            valid = isinstance(spec, dict) and spec.get("qscale", 0) in (0, *range(2, 32)) and 0 <= spec.get("sharpen", 0) <= 64
            if FC.finished(spec) and valid and size is not None:
                assert st == ERR_NO_STAGE and sof is None, (i, q, st)
                assert "no finishing stage" in msg and "kernel library" in msg, msg
                continue
            if FC.finished(spec):  # invalid options: -60 with or without the stage
                assert st == ERR and "qscale 40 (0 or 2..31)" in msg, (i, q, st, msg)
                continue
            # every other rendition: the usual result line, what it is without the finishing ones
            assert (st, sof, msg) == (without["status"][kept_items][q2], without["sof"][kept_items][q2], without["errors"][w]), (i, q)
            q2 += 1
            w += 1
        kept_items += bool(kept)
    st = with_["status"]
    assert st[0] == [0, 0] and st[1] == [0, ERR_NO_STAGE, 0, ERR_NO_STAGE] and st[3] == [ERR, 0] and st[4] == [ERR_NO_STAGE]
    assert st[2][0] not in (0, ERR, ERR_NO_STAGE)  # the malformed stream
    assert with_["sof"][1] == [[416, 240], None, [150, 100], None]
    assert with_["renditions"] == without["renditions"] == 5
    assert (with_["parsed"], without["parsed"]) == (5, 4) and (with_["frames"], without["frames"]) == (3, 3)
    assert dec["error"] is not None and "no finishing stage" in dec["error"] and "(-62)" in dec["error"]


def test_plan_of_a_fixed_chunk(new_dir):
    text, (res,) = run_case(new_dir, "b")
    lines = sections_of(text)["fixed chunk"]
    assert res["status"] == [[0, 0, 0], [0, 0, 0, 0, 0], [0]] and res["renditions"] == 9 and res["frames"] == 3
    assert res["sof"] == [[[36, 20], [72, 40], [72, 40]], [[416, 240], [208, 120], [416, 240], [104, 60], [416, 240]], [[64, 64]]]
    # the launch order: ... sao, scale, finish, then K4 through the entry that takes the scales, then K5
    stages = [l.split()[0] for l in lines if re.match(r"[a-z0-9]+ nframes ", l)]
    assert stages == ["prep", "predict", "deblock", "sao", "scale", "finish", "jpeg", "entropy"], stages
    # the K3u map: grouped by source class, each record with its source's description
    head = [l for l in lines if l.startswith("finish map=")]
    # tiles: 64 dwords x 16 rows a workgroup, luma + 2 chroma planes: 208 x 120: 8 + 2 * 4; 64 x 64: 4 + 2 * 2;
    # 416 x 240: 2 * 15 + 2 * 8
    assert len(head) == 1 and head[0].endswith(" first 0,2,3 count 2,1,1 tiles 16,8,46"), head
    assert [l for l in lines if l.startswith("fin ")] == FC.FIN_B
    # the qforce array: one value a view, in view order
    q = [l for l in lines if l.startswith("qforce=")]
    assert len(q) == 1 and [int(x) for x in q[0].split()[1:]] == FC.QFORCE_B
    assert "jpeg nframes 8 " in "\n".join(lines)
    # both arrays lie in the staging buffer, behind everything else, the qforce array last
    h2d = int(next(l for l in lines if l.startswith("h2d ")).split()[1])
    off_fin, off_q = int(head[0].split()[1][len("map=+"):]), int(q[0].split()[0][len("qforce=+"):])
    assert 0 < off_fin < off_q < h2d and off_fin % 256 == 0 and off_q % 256 == 0
    assert off_q - off_fin >= 4 * 104 and h2d - off_q >= 8 * 4


def test_both_options_zero_is_the_multi4_call(new_dir):
    text, results = run_case(new_dir, "c")
    sections = sections_of(text)
    assert_same(sections, "plain", "zero")
    assert not any(l.startswith(("finish", "qforce")) for l in sections["zero"])
    assert all(st == 0 for r in results for item in r["status"] for st in item)
