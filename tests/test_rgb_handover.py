"""RGB output without a GPU: what the host engine hands to the kernel library when renditions name a format --
against the host-memory stand-in without the stage (tests/fake_gpu/fake_gpu.cpp) and one with it
(tests/fake_gpu/fake_gpu_rgb.cpp), built and selected as test_finish_api.py does it."""
import json
import os
import re
import sys

import pytest

import rgb_handover_cases as RC
from conftest import ROOT
from test_finish_api import IDENT, build_fake
from test_orient_handover import sections_of

ERR, ERR_NO_STAGE = -60, -62


@pytest.fixture(scope="module")
def old_dir(tmp_path_factory):
    return build_fake(tmp_path_factory, "fake_gpu_old_rgb", "fake_gpu.cpp")


@pytest.fixture(scope="module")
def new_dir(tmp_path_factory):
    return build_fake(tmp_path_factory, "fake_gpu_rgb", "fake_gpu_rgb.cpp")


def run_case(lib_dir, case):
    import subprocess
    env = dict(os.environ, H2J_LIB_DIR=lib_dir)
    for k in ("H2J_CHUNK", "H2J_ENGINES", "H2J_STRICT_REFERENCE", "H2J_TAIL", "H2J_TAIL_MIN"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "rgb_handover_cases.py"), case], env=env,
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=120)
    text = p.stderr.decode()
    assert p.returncode == 0, text[-2000:]
    assert text.split("\n", 1)[0] == IDENT, text[:500]
    return text, [json.loads(l[7:]) for l in text.splitlines() if l.startswith("result ")]


def test_raw_rendition_fails_alone_without_the_stage(old_dir):
    text, (res,) = run_case(old_dir, "a")
    st = res["status"]
    assert st[0] == [0, ERR_NO_STAGE] and st[1] == [ERR_NO_STAGE, 0] and st[3] == [ERR, 0] and st[4] == [ERR_NO_STAGE]
    assert st[2][0] not in (0, ERR, ERR_NO_STAGE)  # the malformed stream
    assert res["sof"] == [[[64, 64], None], [None, [208, 120]], [None], [None, [64, 64]], [None]]
    for o in (1, 2, 7):  # output indices: the items have 2, 2, 1, 2, 1 renditions
        assert "no RGB stage" in res["errors"][o] and "h2j_gpu_rgb" in res["errors"][o], res["errors"][o]
    assert "format 1" in res["errors"][5] and "qscale 9" in res["errors"][5]
    assert res["errors"][0] == res["errors"][3] == res["errors"][6] == ""
    assert (res["renditions"], res["frames"], res["parsed"], res["raw_bytes"]) == (3, 3, 5, 0)  # every item had an option set worth parsing for
    assert not any(l.startswith(("rgb ", "px ")) for l in text.splitlines())  # nothing of the stage reaches the library


def test_plan_of_a_fixed_chunk(new_dir):
    text, (res,) = run_case(new_dir, "b")
    lines = sections_of(text)["fixed chunk"]
    assert res["status"] == [[0] * 6, [0, 0], [0, 0]] and res["renditions"] == 10 and res["frames"] == 3
    assert res["sof"] == [[["px", 20, 36, 3], [36, 20], [36, 20], ["px", 3, 40, 72], [72, 40], ["px", 20, 36, 3]],
                          [["px", 60, 104, 3], ["px", 3, 200, 300]], [["px", 64, 64, 3], ["px", 3, 64, 64]]]
    assert res["raw_bytes"] == 2 * 3 * 36 * 20 + 3 * 72 * 40 + 3 * 104 * 60 + 3 * 300 * 200 + 2 * 3 * 64 * 64
    # the launch order: ... scale, finish (the sharpened raw output), rgb, then K4 / K5
    stages = [l.split()[0] for l in lines if re.match(r"[a-z0-9]+ nframes ", l)]
    assert stages == ["prep", "predict", "deblock", "sao", "scale", "finish", "rgb", "jpeg", "entropy"], stages
    # six views: a raw rendition with the geometry of a JPEG rendition reads that rendition's view -- whatever its
    # place in the list and the other's quantiser scale -- so the scale stage has three outputs to make, not five.
    # K4 / K5 run on the three of them that a JPEG rendition shows, with those views' forced scales
    assert "jpeg nframes 3 " in "\n".join(lines) and "entropy nframes 3 " in "\n".join(lines)
    q = [l for l in lines if l.startswith("qforce=")]
    assert len(q) == 1 and [int(x) for x in q[0].split()[1:]] == [0, 0, 7]
    head = [l for l in lines if l.startswith("rgb map=")]
    # tiles: 64 lanes of 4 pixels x 4 lane rows of (2 rows, h / 2 + 1 of them): 104 x 60: 1 x 8; 72 x 40: 6, 64 x 64: 9; 300 x 200: 2 x 26
    assert len(head) == 1 and head[0].endswith(" first 0,2,5 count 2,3,1 tiles 8,9,52"), head
    assert [l for l in lines if l.startswith("px ")] == RC.PX_B
    # the map lies in the staging buffer, behind everything else
    h2d = int(next(l for l in lines if l.startswith("h2d ")).split()[1])
    off = int(head[0].split()[1][len("map=+"):])
    assert 0 < off < h2d and off % 256 == 0 and h2d - off >= 6 * 80
    # one device-to-host copy of the chunk's RGB region: every output from a 256-byte boundary
    region = sum((3 * w * h + 255) // 256 * 256 for w, h in ((36, 20), (72, 40), (104, 60), (300, 200), (64, 64), (64, 64)))
    assert [l for l in lines if l == f"d2h {region}"] == [f"d2h {region}"]


def test_a_chunk_of_raw_renditions_only_runs_no_jpeg_stage(new_dir):
    text, (res,) = run_case(new_dir, "c")
    lines = sections_of(text)["raw only"]
    assert res["status"] == [[0], [0, 0]] and res["sof"] == [[["px", 32, 32, 3]], [["px", 3, 40, 72], ["px", 40, 72, 3]]]
    assert res["raw_bytes"] == 3 * 32 * 32 + 2 * 3 * 72 * 40 and (res["renditions"], res["frames"]) == (3, 2)
    # nobody asked for a JPEG: K4 and K5 are not launched, and no payload is copied -- the downloads are the pool's
    # (cleared) byte count, the jstat records (two views: device-side error flags) and the RGB region
    stages = [l.split()[0] for l in lines if re.match(r"[a-z0-9]+ nframes ", l)]
    assert stages == ["prep", "predict", "deblock", "sao", "scale", "rgb"], stages
    region = sum((3 * w * h + 255) // 256 * 256 for w, h in ((32, 32), (72, 40), (72, 40)))
    d2h = [int(l.split()[1]) for l in lines if l.startswith("d2h ")]
    assert len(d2h) == 3 and d2h[0] == 8 and d2h[2] == region and d2h[1] % 512 == 0, d2h  # (two records of whole 256-byte groups)
    assert "memset 8" in lines
