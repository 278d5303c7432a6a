"""Colour without a GPU: the option word's validity, the multi7 calls' rejection of it, h2j_stream_colour on the
tests/golden/colour vectors and on HEIC files whose nclx property is patched, the exported names, and -- against the
host-memory stand-in with every stage but the colour stage (tests/fake_gpu/fake_gpu_pad.cpp) -- a converted rendition
failing alone and a rendition that resolves to JFIF's being the call without the option (DESIGN.md "Colour (K3v)")."""
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest

import colour_ref as COL
import h2j
import heif_mux as M
from conftest import PKG, ROOT
from test_finish_api import IDENT
from test_pad_handover import build_fake_ext

ERR, ERR_NO_STAGE = -60, -62
GOLDEN = os.path.join(ROOT, "tests", "golden")
AUTO, EXPLICIT = -1, 0x100


def manifest():
    with open(os.path.join(GOLDEN, "colour", "manifest.json")) as f:
        return json.load(f)


def vector(name):
    with open(os.path.join(GOLDEN, "colour", name), "rb") as f:
        return f.read()


def patch_nclx(heic: bytes, primaries, transfer, matrix, full, which=None):
    """The muxed file with the 7 bytes of its nclx colour properties (heif_mux writes 1, 1, 1, full range) replaced."""
    import struct
    key = b"colrnclx"
    at = [m.start() + len(key) for m in re.finditer(re.escape(key), heic)]
    assert at, "no nclx colr property"
    out = bytearray(heic)
    for a in at:
        out[a:a + 7] = struct.pack(">HHHB", primaries, transfer, matrix, 0x80 if full else 0)
    return bytes(out)


def opts8(colour=0, fw=0, fh=0, **kw):
    o = h2j.OutOpts8()
    o.fit_w, o.fit_h, o.colour = fw, fh, colour
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_struct_and_names():
    src = open(os.path.join(ROOT, "include", "h2j.h")).read()
    ext = open(os.path.join(ROOT, "include", "h2j_ext.h")).read()
    m = re.search(r"typedef struct \{([^}]*)\}\s*h2j_out_opts8;", src)
    assert m
    names = [nm.strip() for decl in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(";") if decl.strip()
             for nm in decl.strip()[len("int32_t "):].split(",")]
    assert names == [f for f, _ in h2j.OutOpts8._fields_] and names[-1] == "colour"
    assert ctypes.sizeof(h2j.OutOpts8) == ctypes.sizeof(h2j.OutOpts7) == 64
    assert h2j.OutOpts8.colour.offset == h2j.OutOpts7.reserved.offset == 60
    for fn, _ in h2j.OutOpts7._fields_[:15]:
        assert getattr(h2j.OutOpts7, fn).offset == getattr(h2j.OutOpts8, fn).offset
    assert re.search(r"#define H2J_COLOUR_AUTO \(-1\)", src) and re.search(r"#define H2J_COLOUR_EXPLICIT 0x100", src)
    assert (h2j.COLOUR_AUTO, h2j.COLOUR_EXPLICIT) == (AUTO, EXPLICIT)
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, "libH265ToJpegExt.so")], stdout=subprocess.PIPE, check=True).stdout.decode()
    exported = {f[2] for f in (l.split() for l in out.splitlines()) if len(f) == 3 and f[1] in "TW"}
    for sym in ("h2j_engine_transcode_multi8", "h2j_engine_submit_multi8", "h2j_engine_decode_multi8", "h2j_h265_to_jpeg_mem_multi8",
                "h2j_stream_colour", "h2j_colour_coeffs"):
        assert sym in exported and re.search(r"\b" + sym + r"\(", ext) and hasattr(h2j.load_library(), sym), sym
    assert re.search(r"\bint h2j_gpu_colour\(", open(os.path.join(ROOT, "include", "h2j_gpu.h")).read())
    assert h2j.Engine.stats.__code__ and h2j.STAT_KEYS_COLOUR == ["colour_bytes"]


def test_rendition_spec_shapes():
    rs = h2j.rendition_spec
    assert rs({"fit": (64, 64), "pad": True}) == (0, 0, 64, 64, 0) + (0,) * 8 + (1, 0)   # without the key: what it was
    assert rs({"fit": (64, 64), "colour": ("bt709", "limited")}) == (0, 0, 64, 64, 0) + (0,) * 10 + (EXPLICIT | 1 << 1,)
    assert rs({"colour": "auto", "format": "rgb", "pad": (1, 2, 3), "fit": (8, 8)}) == (0, 0, 8, 8, 0) + (0,) * 7 + (1, 1, 0x010203, AUTO)
    assert rs({"colour": ("bt2020", "full")})[15] == EXPLICIT | 9 << 1 | 1 == COL.word("bt2020", "full")
    assert rs({"colour": ("bt601", "full")})[15] == EXPLICIT | 6 << 1 | 1
    assert rs({"colour": None, "scale": 1}) == (1,) + (0,) * 15
    for bad in ({"colour": "bt709"}, {"colour": ("bt709",)}, {"colour": ("bt709", "wide")}, {"colour": ("rec709", "full")}, {"colour": 1}, {"colour": True}):
        with pytest.raises(ValueError, match="colour"):
            rs(bad)
    nrend, o, total = h2j._multi_opts(h2j.normalize_renditions([0, {"fit": (64, 64), "colour": "auto"}], 2))
    assert o._type_ is h2j.OutOpts8 and total == 4 and (o[1].fit_w, o[1].colour, o[0].colour) == (64, AUTO, 0)
    # specs without colour take the calls they always took
    assert h2j._multi_opts(h2j.normalize_renditions([0, {"fit": (64, 64), "pad": True}], 1))[1]._type_ is h2j.OutOpts7
    assert h2j._multi_opts(h2j.normalize_renditions([0, {"format": "rgb"}], 1))[1]._type_ is h2j.OutOpts6
    assert h2j._multi_opts(h2j.normalize_renditions([0, 1], 1))[1]._type_ is h2j.OutOpts2
    specs = h2j._window_specs(3, None, None, None, False, None, None, colour=["auto", None, ("bt709", "full")])
    assert [rs(s[0])[15:] for s in specs] == [(AUTO,), (), (EXPLICIT | 1 << 1 | 1,)]
    assert [rs(s[0])[15:] for s in h2j._window_specs(2, None, None, None, False, None, None, colour=("bt601", "limited"))] == [(EXPLICIT | 6 << 1,)] * 2
    with pytest.raises(ValueError, match="colour: 2 entries for 3 streams"):
        h2j._window_specs(3, None, None, None, False, None, None, colour=["auto", "auto"])


def test_stream_colour_on_the_vectors():
    seen = set()
    for m in manifest():
        got = h2j.stream_colour(vector(m["file"]))
        assert got == {"primaries": m["primaries"], "transfer": m["transfer"], "matrix": m["matrix"], "full_range": bool(m["full_range"])}, m["file"]
        seen.add((m["codec"], m["bit_depth"], m["matrix"], m["full_range"], m["vui"]))
    assert {(265, 8, 1, 0, True), (265, 10, 9, 0, True), (264, 8, 1, 1, True), (265, 8, 2, 1, True), (264, 8, 2, 0, False), (265, 8, 8, 0, True)} <= seen
    # the older fixtures signal nothing; hevcgen's --vui 1 writes BT.709 full range
    for rel in ("img01.h265", "hevc/p11_64x64_tiny.h265", "h264/a11_64x64_tiny.h264"):
        with open(os.path.join(GOLDEN, rel), "rb") as f:
            assert h2j.stream_colour(f.read()) == {"primaries": 2, "transfer": 2, "matrix": 2, "full_range": False}, rel
    info = (ctypes.c_int32 * 4)(7, 7, 7, 7)
    lib = h2j.load_library()
    assert lib.h2j_stream_colour(h2j._u8(b"not a stream at all, not at all"), 31, info) == -100 and list(info) == [7] * 4
    assert lib.h2j_stream_colour(None, 0, info) == -1 and lib.h2j_stream_colour(h2j._u8(b"x"), 1, None) == -1
    with pytest.raises(ValueError):
        h2j.stream_colour(b"\x00\x00\x00\x01garbage")


def test_stream_colour_on_patched_heics():
    vui709 = vector("c709_limited.hevc")      # VUI: 1, 1, 1, limited
    novui = vector("cnovui.avc")
    heic = M.mux([vui709])
    assert h2j.stream_colour(heic) == {"primaries": 1, "transfer": 1, "matrix": 1, "full_range": True}  # the nclx heif_mux writes wins
    for vals in ((9, 16, 9, 0), (1, 13, 6, 1), (5, 6, 5, 0), (2, 2, 2, 0), (1, 1, 8, 1), (12, 18, 0, 1)):
        got = h2j.stream_colour(patch_nclx(heic, *vals))
        assert (got["primaries"], got["transfer"], got["matrix"], int(got["full_range"])) == vals, vals
    assert h2j.stream_colour(patch_nclx(M.mux([novui], codec=264), 9, 16, 9, 0))["matrix"] == 9
    # a colr that is no nclx is ignored: the item's VUI stands
    prof = heic.replace(b"colrnclx", b"colrprof")
    assert h2j.stream_colour(prof) == {"primaries": 1, "transfer": 1, "matrix": 1, "full_range": False}
    assert h2j.stream_colour(M.mux([novui], codec=264).replace(b"colrnclx", b"colrrICC")) == {"primaries": 2, "transfer": 2, "matrix": 2, "full_range": False}
    # a grid: the grid item has no colr, its tiles' is used
    tiles = []
    for t in range(4):
        with open(os.path.join(GOLDEN, "heif", f"a_{t}.hevc"), "rb") as f:
            tiles.append(f.read())
    with open(os.path.join(GOLDEN, "heif", "manifest.json")) as f:
        a = next(s for s in json.load(f) if s["set"] == "a")
    grid = M.mux(tiles, grid=(2, 2, 2 * a["tile_w"], 2 * a["tile_h"]), tile_size=(a["tile_w"], a["tile_h"]))
    assert h2j.stream_colour(grid)["matrix"] == 1 and h2j.stream_colour(grid)["full_range"] is True
    got = h2j.stream_colour(patch_nclx(grid, 9, 14, 9, 0))
    assert (got["primaries"], got["transfer"], got["matrix"], got["full_range"]) == (9, 14, 9, False)
    assert h2j.stream_colour(grid.replace(b"colrnclx", b"colrprof")) == {"primaries": 2, "transfer": 2, "matrix": 2, "full_range": False}


# ---- against the stand-in kernel library, which has no h2j_gpu_colour

@pytest.fixture(scope="module")
def old_dir(tmp_path_factory):
    return build_fake_ext(tmp_path_factory, "fake_gpu_old_colour", "fake_gpu_pad.cpp")


def run_case(lib_dir, case):
    env = dict(os.environ, H2J_LIB_DIR=lib_dir)
    for k in ("H2J_CHUNK", "H2J_ENGINES", "H2J_STRICT_REFERENCE", "H2J_TAIL", "H2J_TAIL_MIN"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "colour_handover_cases.py"), case], env=env,
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=120)
    text = p.stderr.decode()
    assert p.returncode == 0, text[-2000:]
    assert text.split("\n", 1)[0] == IDENT, text[:500]
    return text, [json.loads(l[7:]) for l in text.splitlines() if l.startswith("result ")]


def test_validity_grid_of_the_word(old_dir):
    """Every value of the word through h2j_engine_transcode_multi8, one item each: an invalid one fails its rendition
    alone with H2J_ERR_OUT_OPTS; a valid one resolves -- to JFIF's (0, or BT.601 full range: the JPEG) or to a source the
    stand-in has no stage for.  The multi7 calls keep rejecting a non-zero word in that place."""
    import colour_handover_cases as C
    _, (r8, r7) = run_case(old_dir, "v")
    assert len(C.WORDS) > 100 and len(r8["status"]) == len(C.WORDS)
    jfif = (0, EXPLICIT | 6 << 1 | 1, EXPLICIT | 5 << 1 | 1)
    for w, st, err in zip(C.WORDS, r8["status"], r8["errors"]):
        want = 0 if w in jfif else ERR_NO_STAGE if w in C.VALID else ERR
        assert st == want, (w, st, err)
        if want == ERR and w != -(1 << 31):
            assert f"colour {w} " in err, (w, err)
    assert r7["status"] == [ERR] * len(C.WORDS7) and all("reserved non-zero" in e for e in r7["errors"]), r7


def test_converted_rendition_fails_alone_without_the_stage(old_dir):
    text, (res,) = run_case(old_dir, "a")
    st = res["status"]
    assert st[0] == [0, ERR_NO_STAGE] and st[1] == [ERR_NO_STAGE] and st[2] == [0, 0, ERR_NO_STAGE] and st[3] == [ERR, 0, ERR_NO_STAGE], st
    assert st[4][0] not in (0, ERR, ERR_NO_STAGE)  # the malformed stream
    # a source that is JFIF's already is the job without colour: it needs no stage
    assert res["sof"] == [[[64, 64], None], [None], [[64, 64], ["px", 64, 64, 3], None], [None, [64, 64], None], [None]]
    for o in (1, 2, 5, 8):  # output indices: the items have 2, 1, 3, 3, 1 renditions
        assert "no colour stage" in res["errors"][o] and "h2j_gpu_colour" in res["errors"][o], res["errors"][o]
    assert "scale_log2 7" in res["errors"][6] and "colour 258" in res["errors"][6]
    assert res["errors"][0] == res["errors"][3] == res["errors"][4] == res["errors"][7] == ""
    assert (res["renditions"], res["frames"], res["parsed"], res["colour_bytes"]) == (4, 3, 5, 0)
    # the stage is reported after orient and before finish: a rendition that needs all three is told of the colour stage
    # by a library that has the other two


def test_a_source_that_is_jfif_hands_over_what_the_call_without_colour_does(old_dir):
    with_colour, (a,) = run_case(old_dir, "b")
    without, (b,) = run_case(old_dir, "c")
    assert a == b and a["colour_bytes"] == 0 and a["status"] == [[0, 0, 0], [0], [0, 0]]
    assert with_colour == without and len(with_colour.splitlines()) > 20  # every digest, offset and stage line
