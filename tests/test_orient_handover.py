"""Oriented output on the host, without a GPU: libH265ToJpeg.so against the host-memory stand-in for
libh2j_hip.so (tests/fake_gpu/fake_gpu.cpp), built and selected as test_crop_handover.py does it.  The
stand-in has no h2j_gpu_orient, as a kernel library older than the orientation stage.

- Renditions whose orientation resolves to 0 (orient 0, 1, or auto on a stream without the SEI) hand the GPU
  exactly what the same call without an orientation hands it: the transcripts are compared inside the run.
- A display orientation SEI in the stream changes nothing of what is handed over when no rendition asks for it.
- An oriented rendition fails alone with -62 on such a kernel library; everything else is what it is without it.
The recorded transcripts of the existing calls are test_engine_handover.py's to check.
"""
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

import handover_cases as H
import orient_handover_cases as C
from conftest import PKG, ROOT

ERR_OUT_OPTS, ERR_NO_STAGE = -60, -62
IDENT = "fake_gpu: host-memory stand-in for libh2j_hip.so"


@pytest.fixture(scope="module")
def fake_dir(tmp_path_factory):
    host = os.path.join(PKG, "libH265ToJpeg.so")
    assert os.path.exists(host), f"{host} is not built: run __graft_entry__.build() first"
    d = str(tmp_path_factory.mktemp("fake_gpu_orient"))
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-shared", "-fPIC", "-Wall",
                           "-I" + os.path.join(ROOT, "include"), "-o", os.path.join(d, "libh2j_hip.so"),
                           os.path.join(ROOT, "tests", "fake_gpu", "fake_gpu.cpp")])
    shutil.copy(host, d)
    return d


_runs = {}


def run_case(fake_dir, case):
    if case not in _runs:
        env = dict(os.environ, H2J_LIB_DIR=fake_dir, **C.ENV.get(case, {}))
        for k in ("H2J_CHUNK", "H2J_ENGINES", "H2J_STRICT_REFERENCE", "H2J_TAIL", "H2J_TAIL_MIN"):
            if k not in C.ENV.get(case, {}):
                env.pop(k, None)
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "orient_handover_cases.py"), case], env=env,
                           stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=120)
        text = p.stderr.decode()
        assert p.returncode == 0, text[-2000:]
        assert text.split("\n", 1)[0] == IDENT, text[:500]
        _runs[case] = (text, [json.loads(l[7:]) for l in text.splitlines() if l.startswith("result ")])
    return _runs[case]


def sections_of(text):
    sections, cur = {}, None
    for line in text.splitlines()[1:]:
        if line.startswith("== "):
            cur = line[3:]
            sections[cur] = []
        elif cur is not None:
            sections[cur].append(line)
    return sections


def renumbered(lines):
    # the stand-in numbers event records over the whole process: count from the call's first record
    base = next(int(l.split("#")[1]) for l in lines if l.startswith("record #")) - 1
    return [re.sub(r"#(\d+)", lambda m: "#" + str(int(m.group(1)) - base if int(m.group(1)) else 0), l) for l in lines]


def assert_same(sections, a, b):
    x, y = renumbered(sections[a]), renumbered(sections[b])
    assert any(l.startswith("h2d ") for l in x) and any(l.startswith("result ") for l in x)
    first = next((i for i, (p, q) in enumerate(zip(x, y)) if p != q), None)
    assert x == y, f"{a} / {b}: transcripts differ at line {first}: {x[first]} vs {y[first]}"


def test_orientation_zero_is_no_orientation(fake_dir):
    text, results = run_case(fake_dir, "a")
    sections = sections_of(text)
    assert len(sections) == 2 * len(C.SAME_A) and len(results) == 2 * len(C.SAME_A)
    for k in range(len(C.SAME_A)):
        assert_same(sections, f"{k} plain", f"{k} orient")
        assert any(l.startswith("scale ") for l in sections[f"{k} plain"])
    assert all(st == 0 for r in results for item in r["status"] for st in item)


def test_oriented_rendition_fails_alone_without_the_stage(fake_dir):
    with_, without, dec = run_case(fake_dir, "b")[1]
    o, w = 0, 0  # output indices with / without the oriented renditions
    kept_items = 0
    for i, (idx, specs) in enumerate(C.ITEMS_B):
        size = H.POOL[idx][1]
        kept = C.without_oriented(specs)
        q2 = 0
        for q, spec in enumerate(specs):
            st, sof, msg = with_["status"][i][q], with_["sof"][i][q], with_["errors"][o]
            o += 1
            if isinstance(spec, dict) and 2 <= spec.get("orient", 0) <= 8 and size is not None:
                assert st == ERR_NO_STAGE and sof is None, (i, q, st)
                assert "no orientation stage" in msg and "kernel library" in msg, msg
                continue
            # every other rendition: what it is without the oriented ones
            assert (st, sof, msg) == (without["status"][kept_items][q2], without["sof"][kept_items][q2], without["errors"][w]), (i, q)
            q2 += 1
            w += 1
        kept_items += bool(kept)
    st = with_["status"]
    assert st[0] == [0, 0] and st[1] == [0, ERR_NO_STAGE, 0] and st[3] == [ERR_OUT_OPTS, 0] and st[4] == [ERR_NO_STAGE]
    assert st[2][0] not in (0, ERR_OUT_OPTS, ERR_NO_STAGE)  # the malformed stream
    assert "orient 9" in with_["errors"][6] and with_["errors"][6].startswith("invalid output options: scale_log2 0 (0..3)")
    assert with_["sof"][1] == [[416, 240], None, [150, 100]]
    assert with_["renditions"] == without["renditions"] == 5
    assert (with_["parsed"], without["parsed"]) == (5, 4) and (with_["frames"], without["frames"]) == (3, 3)
    assert dec["error"] is not None and "no orientation stage" in dec["error"] and "(-62)" in dec["error"]


def test_sei_in_the_stream_changes_nothing_unasked(fake_dir):
    text, (plain, sei, bad) = run_case(fake_dir, "c")
    assert_same({k: [l for l in v if not l.startswith("result ")] + ["result same"] for k, v in sections_of(text).items()}, "plain", "sei")
    assert plain["orientation"] == [0, 0, 0] and sei["orientation"] == [5, 7, 4]
    assert plain["status"] == sei["status"] == [[0, 0]] * 3 and plain["sof"] == sei["sof"]
    assert bad["status"] == [[0], [0]] and bad["sof"] == [[[64, 64]], [[64, 64]]]
