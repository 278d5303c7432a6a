"""HEIF input and what the host engine hands to the GPU library, checked without a GPU (the stand-in and the
conventions of test_engine_handover.py).

A batch of [Annex-B stream, single-item HEIC of the same stream] must hand over two identical pictures: its transcript
(sizes, digest of the staging bytes, every stage's descriptor) is the transcript of the batch [stream, stream].  And no
stream under tests/golden/ is taken for a HEIF file, so every Annex-B input goes down the path it always went."""
import glob
import os
import re
import shutil
import subprocess
import sys

import pytest

import heif_host_build as B
from conftest import GOLDEN, PKG, ROOT

IDENT = "fake_gpu: host-memory stand-in for libh2j_hip.so"


@pytest.fixture(scope="module")
def transcript(tmp_path_factory):
    host = os.path.join(PKG, "libH265ToJpeg.so")
    assert os.path.exists(host), f"{host} is not built: run __graft_entry__.build() first"
    d = str(tmp_path_factory.mktemp("fake_gpu_heif"))
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-shared", "-fPIC", "-Wall",
                           "-I" + os.path.join(ROOT, "include"), "-o", os.path.join(d, "libh2j_hip.so"),
                           os.path.join(ROOT, "tests", "fake_gpu", "fake_gpu.cpp")])
    shutil.copy(host, d)
    env = dict(os.environ, H2J_LIB_DIR=d)
    for k in ("H2J_CHUNK", "H2J_ENGINES", "H2J_STRICT_REFERENCE", "H2J_TAIL", "H2J_TAIL_MIN"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "heif_handover_child.py")], env=env,
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=120)
    text = p.stderr.decode()
    assert p.returncode == 0, text[-2000:]
    assert text.split("\n", 1)[0] == IDENT, text[:500]
    calls = {}
    for part in text.split("\n== ")[1:]:
        label, _, body = part.partition("\n")
        # the stand-in numbers events over the life of the process: renumbered from each call's first
        ids = {}
        calls[label] = re.sub(r"#(\d+)", lambda m: "#" + str(ids.setdefault(m.group(1), len(ids))), body.rstrip("\n"))
    return calls


def test_heic_item_hands_over_the_streams_picture(transcript):
    names = sorted({k.split(": ")[0] for k in transcript})
    assert len(names) == 3
    for n in names:
        want = transcript[f"{n}: annexb twice"]
        assert "result " in want and '"status": [0, 0]' in want, want[-300:]
        assert len(want.splitlines()) > 5  # the stand-in's record of copies and stages is there
        assert transcript[f"{n}: annexb and heic"] == want, n
        assert transcript[f"{n}: heic twice"] == want, n


def test_no_golden_stream_is_taken_for_heif(tmp_path):
    exe = B.build(tmp_path)
    paths = sorted(p for pat in ("*.h264", "*.h265", "*.hevc", "*.avc") for p in glob.glob(os.path.join(GOLDEN, "**", pat), recursive=True))
    assert len(paths) >= 280
    out = subprocess.check_output([exe, "probe"] + paths, text=True).split()
    assert out == ["0"] * len(paths)
