"""Padded output without a GPU: what the host engine hands to the kernel library when renditions name `pad` -- against
the host-memory stand-in with every stage but the padding stage (tests/fake_gpu/fake_gpu_orient.cpp) and one with it
(tests/fake_gpu/fake_gpu_pad.cpp), built and selected as test_rgb_handover.py does it."""
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

import pad_ref as PAD
import test_handover_recorded as REC
from conftest import PKG, ROOT
from pad_handover_cases import GREY, RED
from test_finish_api import IDENT, build_fake
from test_orient_handover import sections_of

ERR, ERR_NO_STAGE = -60, -62


def build_fake_ext(tmp_path_factory, name, source):
    """build_fake, with the library that exports the padded output entry points beside the host library."""
    d = build_fake(tmp_path_factory, name, source)
    ext = os.path.join(PKG, "libH265ToJpegExt.so")
    assert os.path.exists(ext), f"{ext} is not built: run __graft_entry__.build() first"
    shutil.copy(ext, d)
    return d


@pytest.fixture(scope="module")
def old_dir(tmp_path_factory):
    return build_fake_ext(tmp_path_factory, "fake_gpu_old_pad", "fake_gpu_orient.cpp")


@pytest.fixture(scope="module")
def new_dir(tmp_path_factory):
    return build_fake_ext(tmp_path_factory, "fake_gpu_pad", "fake_gpu_pad.cpp")


def run_case(lib_dir, case):
    env = dict(os.environ, H2J_LIB_DIR=lib_dir)
    for k in ("H2J_CHUNK", "H2J_ENGINES", "H2J_STRICT_REFERENCE", "H2J_TAIL", "H2J_TAIL_MIN"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "pad_handover_cases.py"), case], env=env,
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=120)
    text = p.stderr.decode()
    assert p.returncode == 0, text[-2000:]
    assert text.split("\n", 1)[0] == IDENT, text[:500]
    return text, [json.loads(l[7:]) for l in text.splitlines() if l.startswith("result ")]


def test_padded_rendition_fails_alone_without_the_stage(old_dir):
    text, (res,) = run_case(old_dir, "a")
    st = res["status"]
    assert st[0] == [0, ERR_NO_STAGE] and st[1] == [ERR_NO_STAGE] and st[2] == [0, 0] and st[3] == [ERR, 0, ERR], st
    assert st[4][0] not in (0, ERR, ERR_NO_STAGE)  # the malformed stream
    # a box the picture part fills is the job without pad: it needs no stage
    assert res["sof"] == [[[64, 64], None], [None], [[64, 64], ["px", 64, 64, 3]], [None, [64, 64], None], [None]]
    for o in (1, 2):  # output indices: the items have 2, 1, 2, 3, 1 renditions
        assert "no padding stage" in res["errors"][o] and "h2j_gpu_pad" in res["errors"][o], res["errors"][o]
    assert "pad 1 (0..1; needs a box" in res["errors"][5] and "background 0" in res["errors"][5]
    assert "scale_log2 1" in res["errors"][7] and "pad 1" in res["errors"][7]
    assert res["errors"][0] == res["errors"][3] == res["errors"][4] == res["errors"][6] == ""
    assert (res["renditions"], res["frames"], res["parsed"], res["pad_bytes"]) == (4, 3, 5, 0)
    assert not any(l.startswith(("pad ", "box ")) for l in text.splitlines())  # nothing of the stage reaches the library


def test_plan_of_a_fixed_chunk(new_dir):
    text, (res,) = run_case(new_dir, "b")
    lines = sections_of(text)["fixed chunk"]
    assert res["status"] == [[0] * 4, [0], [0, 0]] and res["renditions"] == 7 and res["frames"] == 3
    # SOF0 and the raw shapes carry the canvas
    assert res["sof"] == [[[50, 50], ["px", 50, 50, 3], [50, 26], [50, 50]], [["px", 3, 300, 500]], [[70, 66], [64, 64]]]
    assert res["raw_bytes"] == 3 * 50 * 50 + 3 * 500 * 300
    canvases = ((64, 32, 50), (64, 32, 50), (512, 256, 300), (80, 48, 66))  # luma pitch, chroma pitch, rows
    assert res["pad_bytes"] == sum(yl * h + 2 * cl * (h // 2) for yl, cl, h in canvases)
    # the launch order: ... scale, finish (the sharpened picture part), pad, rgb (the raw canvases), then K4 / K5
    stages = [l.split()[0] for l in lines if re.match(r"[a-z0-9]+ nframes ", l)]
    assert stages == ["prep", "predict", "deblock", "sao", "scale", "finish", "pad", "rgb", "jpeg", "entropy"], stages
    # eight views.  K4 / K5 run on five: P12's fit (the unpadded rendition shows it: one picture view for it and three
    # padded renditions) and its two canvases, A11's plain view and its canvas -- not on P04's picture part and canvas
    # (a raw rendition only) nor on A11's sharpened picture part (only a padded rendition shows it)
    assert "jpeg nframes 5 " in "\n".join(lines) and "entropy nframes 5 " in "\n".join(lines)
    q = [l for l in lines if l.startswith("qforce=")]
    assert len(q) == 1 and [int(x) for x in q[0].split()[1:]] == [0, 0, 0, 0, 7]
    head = [l for l in lines if l.startswith("pad map=")]
    # tiles: 64 dwords x 16 rows of the rows' whole 16-byte groups: 50 x 50: 4 + 2 x 2; 70 x 66: 5 + 2 x 3; 500 x 300: 2 x 19 + 2 x 10
    assert len(head) == 1 and head[0].endswith(" first 0,3,3 count 3,0,1 tiles 11,0,58"), head
    box = [l for l in lines if l.startswith("box ")]
    fill = lambda c: "%d,%d,%d" % PAD.pad_colour(c)
    want = [f"box 50 26 in 50 50 at 0,12 fill {fill(GREY)} depth 8,8 wide 1 crop 0,0 pitch 64/64,32,32 at 0,3200,4000",
            "box 50 26 in 50 50 at 0,12 fill 0,128,128 depth 8,8 wide 1 crop 0,0 pitch 64/64,32,32 at 0,3200,4000",
            f"box 64 64 in 70 66 at 2,0 fill {fill(RED)} depth 8,8 wide 1 crop 0,0 pitch 64/80,48,48 at 0,5280,6864",
            "box 416 240 in 500 300 at 42,30 fill 0,128,128 depth 10,10 wide 0 crop 0,0 pitch 416/512,256,256 at 0,153600,192000"]
    assert [l.split(" src ")[0] for l in box] == want, box
    assert fill(GREY) == "114,128,128"
    src = [int(l.split(" src ")[1].split()[0]) for l in box]
    dst = [int(l.split(" dst ")[1]) for l in box]
    assert src[0] == src[1] and len(set(src)) == 3  # one picture view under both of P12's canvases
    assert len(set(dst)) == 4 and all(d % 256 == 0 for d in dst) and not set(dst) & set(src)
    # one canvas for the JPEG and the raw rendition of the same letterbox: K3c has two records, both canvases (wide)
    px = [l for l in lines if l.startswith("px ")]
    assert [l.split(" base ")[0] for l in px] == ["px 50 50 layout 1 depth 8,8 wide 1 crop 0,0 pitch 64,32,32",
                                                 "px 500 300 layout 2 depth 8,8 wide 1 crop 0,0 pitch 512,256,256"], px
    # the map lies in the staging buffer, behind everything else
    h2d = int(next(l for l in lines if l.startswith("h2d ")).split()[1])
    off = int(head[0].split()[1][len("map=+"):])
    others = [int(m) for l in lines for m in re.findall(r"=\+(\d+)", l)]
    assert 0 < off < h2d and off % 256 == 0 and off == max(others) and 4 * 120 <= h2d - off < 4 * 120 + 512


def test_the_largest_canvas_and_the_smallest_box_above_it(new_dir):
    text, (res,) = run_case(new_dir, "c")
    lines = sections_of(text)["largest canvas"]
    assert res["status"] == [[0, ERR, 0, ERR, ERR, 0]], res["status"]
    assert res["sof"] == [[[8192, 8192], None, [65534, 1024], None, None, [64, 64]]]
    for o in (1, 3, 4):
        assert "of at most 67108864 samples" in res["errors"][o], res["errors"][o]
    # (tiles: 8192 x 8192: 32 x 512 + 2 x 16 x 256 workgroups; 65534 x 1024: 256 x 64 + 2 x 128 x 32)
    # the accepted canvases' records: every plane offset and pitch positive, the planes inside 2^27 bytes
    box = [l for l in lines if l.startswith("box ")]
    assert [l.split(" src ")[0] for l in box] == [
        "box 64 64 in 8192 8192 at 4064,4064 fill 0,128,128 depth 8,8 wide 0 crop 0,0 pitch 64/8192,4096,4096 at 0,67108864,83886080",
        "box 64 64 in 65534 1024 at 32734,480 fill 114,128,128 depth 8,8 wide 0 crop 0,0 pitch 64/65536,32768,32768 at 0,67108864,83886080"], box
    assert res["pad_bytes"] == 2 * (67108864 + 2 * 16777216) and (res["renditions"], res["frames"]) == (3, 1)
    head = [l for l in lines if l.startswith("pad map=")]
    assert len(head) == 1 and head[0].endswith(" first 0,0,2 count 0,2,0 tiles 0,24576,0"), head


@pytest.mark.parametrize("module,case", [("rgb", "b"), ("orient", "d"), ("finish", "a"), ("crop", "b")])
def test_a_chunk_without_pad_hands_over_the_recorded_bytes(new_dir, module, case):
    """The recordings of test_handover_recorded.py (staging digests, offsets, descriptors, event order) against a kernel
    library that has the padding stage: chunks that do not ask for it are handed what they always were."""
    with open(REC.recording(module, case, "all")) as f:
        want = REC.expanded(f.read())
    assert REC.transcript(new_dir, module, case) == want
