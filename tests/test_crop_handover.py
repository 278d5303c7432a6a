"""Crop and cover on the host, without a GPU: libH265ToJpeg.so against the host-memory stand-in for
libh2j_hip.so (tests/fake_gpu/fake_gpu.cpp), built and selected as test_engine_handover.py does it.

- SOF sizes of crop, cover and windowed-scale renditions follow the rule (tests/crop_ref.py).
- Invalid renditions fail alone with -60 and a message that names the picture's size.
- A window that resolves to the whole picture hands the GPU exactly what the call without a window hands
  it: the two transcripts (staging digest, descriptors, copies) are compared inside the run.
The recorded transcripts of the existing calls are test_engine_handover.py's to check.
"""
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

import crop_handover_cases as C
import crop_ref
import handover_cases as H
from conftest import PKG, ROOT

ERR_OUT_OPTS = -60
IDENT = "fake_gpu: host-memory stand-in for libh2j_hip.so"


@pytest.fixture(scope="module")
def fake_dir(tmp_path_factory):
    host = os.path.join(PKG, "libH265ToJpeg.so")
    assert os.path.exists(host), f"{host} is not built: run __graft_entry__.build() first"
    d = str(tmp_path_factory.mktemp("fake_gpu_crop"))
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
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "crop_handover_cases.py"), case], env=env,
                           stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=120)
        text = p.stderr.decode()
        assert p.returncode == 0, text[-2000:]
        assert text.split("\n", 1)[0] == IDENT, text[:500]
        _runs[case] = (text, [json.loads(l[7:]) for l in text.splitlines() if l.startswith("result ")])
    return _runs[case]


def test_window_sizes_and_lone_failures(fake_dir):
    (r,) = run_case(fake_dir, "a")[1]
    o, good, invalid = 0, 0, 0
    for i, (idx, specs) in enumerate(C.ITEMS_A):
        size = H.POOL[idx][1]
        assert len(r["status"][i]) == len(specs)
        for q, spec in enumerate(specs):
            st, sof, msg = r["status"][i][q], r["sof"][i][q], r["errors"][o]
            o += 1
            if size is None:  # the parse failure fails every rendition
                assert st not in (0, ERR_OUT_OPTS) and sof is None
                continue
            want = crop_ref.resolve(size[0], size[1], **crop_ref.spec_fields(spec))
            if want is None:
                assert st == ERR_OUT_OPTS and sof is None, (i, q)
                assert "invalid output options" in msg and f"the picture is {size[0]} x {size[1]}" in msg, msg
                invalid += 1
            else:
                assert st == 0 and sof == list(want[1]) and msg == "", (i, q, sof, want)
                good += 1
    assert invalid == 8 and good == 17
    assert r["renditions"] == good and r["parsed"] == len(C.ITEMS_A)
    # the worked sizes: a 1 x 1 chroma window; the 2:1 cover of a right-hand part
    assert r["sof"][0][1] == [2, 2] and r["sof"][1][5] == [50, 100]


def test_whole_picture_window_is_no_window(fake_dir):
    text, results = run_case(fake_dir, "b")
    sections, cur = {}, None
    for line in text.splitlines()[1:]:
        if line.startswith("== "):
            cur = line[3:]
            sections[cur] = []
        elif cur is not None:
            sections[cur].append(line)
    assert len(sections) == 2 * len(C.SAME_B) and len(results) == 2 * len(C.SAME_B)
    def renumbered(lines):
        # the stand-in numbers event records over the whole process: count from the call's first record
        base = next(int(l.split("#")[1]) for l in lines if l.startswith("record #")) - 1
        return [re.sub(r"#(\d+)", lambda m: "#" + str(int(m.group(1)) - base if int(m.group(1)) else 0), l) for l in lines]

    for k in range(len(C.SAME_B)):
        plain, window = renumbered(sections[f"{k} plain"]), renumbered(sections[f"{k} window"])
        assert any(l.startswith("h2d ") for l in plain) and any(l.startswith("scale ") for l in plain)
        first = next((i for i, (a, b) in enumerate(zip(plain, window)) if a != b), None)
        assert plain == window, f"call {k}: transcripts differ at line {first}: {plain[first]} vs {window[first]}"


def test_facade_and_inspection_entry_points(fake_dir):
    mem, dec = run_case(fake_dir, "c")[1]
    assert mem["rc"] == 0 and mem["status"] == [0, 0, ERR_OUT_OPTS, 0]
    assert mem["sof"] == [[300, 200], [64, 64], None, [208, 120]]
    # level 2 of window A's pyramid; the whole-picture level 1 beside it is K3s's
    assert dec == {"size": [76, 50], "mode": 5, "window": [36, 10, 300, 200], "shape": [50, 76]}


def test_items_whose_renditions_all_lie_outside_the_picture(fake_dir):
    """A rendition that fails only after the parse fails alone even when it is the item's only one, or when
    every rendition of the item does: the item gets no frame, its siblings' and neighbours' JPEGs are made."""
    *calls, kw = run_case(fake_dir, "d")[1]
    assert len(calls) == len(C.CALLS_D)
    for r, (idx, rend) in zip(calls, C.CALLS_D):
        o, frames, good = 0, 0, 0
        for i, (pi, specs) in enumerate(zip(idx, rend)):
            size = H.POOL[pi][1]
            wants = [crop_ref.resolve(size[0], size[1], **crop_ref.spec_fields(sp)) for sp in specs]
            frames += any(w is not None for w in wants)
            for q, want in enumerate(wants):
                st, sof, msg = r["status"][i][q], r["sof"][i][q], r["errors"][o]
                o += 1
                if want is None:
                    assert st == ERR_OUT_OPTS and sof is None and f"the picture is {size[0]} x {size[1]}" in msg, (i, q, st, msg)
                else:
                    assert st == 0 and sof == list(want[1]) and msg == "", (i, q)
                    good += 1
        assert (r["frames"], r["renditions"], r["parsed"]) == (frames, good, len(idx))
    assert [c["frames"] for c in calls] == [0, 2, 1, 0]
    assert kw["status"] == [ERR_OUT_OPTS, 0] and kw["sof"] == [None, [72, 40]]
