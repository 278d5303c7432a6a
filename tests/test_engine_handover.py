"""What the host engine hands to the GPU library, checked without a GPU.

libH265ToJpeg.so runs against a host-memory stand-in for libh2j_hip.so (tests/fake_gpu/fake_gpu.cpp) that
runs no kernel and writes a transcript of every copy, memset and stage call: the sizes, a digest of the
staging bytes (the h2j_frame records with all arena offsets, every map, the views, scale_map, pyr_map) and
each stage's descriptor.  A wrong K1 map order or a changed arena layout still gives correct JPEGs on the
GPU; here it changes a digest.

The transcripts under golden/engine_handover/ were recorded once, before the engine's host code was
reorganised, and are never regenerated from the code under test: a difference means the engine now hands
the GPU something else, and a missing file fails the test.

Each case runs in a fresh child python (the pytest process may hold the real GPU library) that finds the
stand-in through H2J_LIB_DIR and the RUNPATH ($ORIGIN) of the copied libH265ToJpeg.so.
"""
import json
import os
import shutil
import subprocess
import sys

import pytest

import handover_cases as H
import resize_ref
import scale_ref
from conftest import PKG, ROOT, golden

ERR_OUT_OPTS = -60  # include/h2j.h H2J_ERR_OUT_OPTS
IDENT = "fake_gpu: host-memory stand-in for libh2j_hip.so"


@pytest.fixture(scope="module")
def fake_dir(tmp_path_factory):
    host = os.path.join(PKG, "libH265ToJpeg.so")
    assert os.path.exists(host), f"{host} is not built: run __graft_entry__.build() first"
    d = str(tmp_path_factory.mktemp("fake_gpu"))
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-shared", "-fPIC", "-Wall",
                           "-I" + os.path.join(ROOT, "include"), "-o", os.path.join(d, "libh2j_hip.so"),
                           os.path.join(ROOT, "tests", "fake_gpu", "fake_gpu.cpp")])
    shutil.copy(host, d)
    return d


_runs = {}


def run_case(fake_dir, case):
    """(transcript, results): the child's stderr, and its `result` lines parsed."""
    if case not in _runs:
        env = dict(os.environ, H2J_LIB_DIR=fake_dir, **H.ENV.get(case, {}))
        for k in ("H2J_CHUNK", "H2J_ENGINES", "H2J_STRICT_REFERENCE", "H2J_TAIL", "H2J_TAIL_MIN"):
            if k not in H.ENV.get(case, {}):
                env.pop(k, None)
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "handover_cases.py"), case], env=env,
                           stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=120)
        text = p.stderr.decode()
        assert p.returncode == 0, text[-2000:]
        # the child ran on the stand-in: the real library prints no such line
        assert text.split("\n", 1)[0] == IDENT, text[:500]
        _runs[case] = (text, [json.loads(l[7:]) for l in text.splitlines() if l.startswith("result ")])
    return _runs[case]


@pytest.mark.parametrize("case", sorted(H.CASES))
def test_transcript_matches_recording(fake_dir, case):
    text, _ = run_case(fake_dir, case)
    path = golden(os.path.join("engine_handover", case + ".txt"))
    assert os.path.exists(path), f"{path} is missing: recordings come from the commit before the refactor, not from this code"
    with open(path) as f:
        want = f.read()
    got_l, want_l = text.splitlines(), want.splitlines()
    first = next((i for i, (a, b) in enumerate(zip(got_l, want_l)) if a != b), min(len(got_l), len(want_l)))
    assert text == want, (f"transcript differs from the recording at line {first + 1}: "
                          f"{got_l[first:first + 1]} vs recorded {want_l[first:first + 1]}")


# ---- the output sizes by the documented rule (h2j_scaled_dim, h2j_fit_size), independent of the recording


def rule_size(size, scale=0, max_dim=0, fit=None, stretch=False):
    w, h = size
    if fit is not None:
        return list(resize_ref.fit_size(w, h, (fit[0] or 0, fit[1] or 0), stretch))
    return list(scale_ref.scaled_size(w, h, scale_ref.resolve_scale(w, h, scale, max_dim)))


def spec_size(size, spec):
    if isinstance(spec, int):
        return rule_size(size, scale=spec)
    if isinstance(spec, tuple):
        return rule_size(size, fit=spec)
    return rule_size(size, spec.get("scale", 0), spec.get("max_dim", 0), spec.get("fit"), spec.get("stretch", False))


def test_pool_sizes(fake_dir):
    (r,) = run_case(fake_dir, "a")[1]
    for i, (_, size) in enumerate(H.POOL):
        assert (r["status"][i] == 0) == (size is not None)
        assert r["sof"][i] == (list(size) if size else None)
    assert r["status"][H.BAD] != ERR_OUT_OPTS


def test_per_item_option_sizes(fake_dir):
    (r,) = run_case(fake_dir, "b")[1]
    for i, ((_, size), (scale, max_dim, fit, stretch)) in enumerate(zip(H.POOL, H.OPTS_B)):
        if i == H.A11:  # the invalid option set
            assert r["status"][i] == ERR_OUT_OPTS and r["sof"][i] is None
        elif size is None:
            assert r["status"][i] not in (0, ERR_OUT_OPTS) and r["sof"][i] is None
        else:
            assert r["status"][i] == 0
            assert r["sof"][i] == rule_size(size, scale, max_dim, fit, stretch), i
    assert r["sof"][H.P4K] == [1920, 1080] and r["sof"][H.P04] == [104, 60]  # the K3s fit; max_dim


def test_rendition_sizes(fake_dir):
    (r,) = run_case(fake_dir, "c")[1]
    invalid = {(H.P19, 1), (H.P4K, 0), (H.P4K, 1)}
    nrend = 0
    for i, ((_, size), specs) in enumerate(zip(H.POOL, H.RENDS_C)):
        assert len(r["status"][i]) == len(r["sof"][i]) == len(specs)
        for q, spec in enumerate(specs):
            st, sof = r["status"][i][q], r["sof"][i][q]
            if size is None:  # the parse failure fails every rendition
                assert st not in (0, ERR_OUT_OPTS) and sof is None
            elif (i, q) in invalid:
                assert st == ERR_OUT_OPTS and sof is None
            else:
                assert st == 0 and sof == spec_size(size, spec), (i, q)
                nrend += 1
    # the item whose renditions are all invalid is not parsed; the malformed one is (its parse ran)
    assert r["parsed"] == len(H.POOL) - 1
    assert r["renditions"] == nrend


def test_single_picture_entry_points(fake_dir):
    dec, batch, coeffs, scaled, resized, multi = run_case(fake_dir, "d")[1]
    assert dec == {"shape": [40, 72], "bit_depth": 8}
    assert batch == {"shape": [64, 64], "bit_depth": 8}  # pick 1: the H.264 tiny picture
    assert coeffs == {"shape": [(352 // 16) * (288 // 16), 6, 64]}
    assert scaled == {"shape": [60, 104], "scale": 2}
    assert resized["shape"] == rule_size((480, 272), fit=(100, 0))[::-1]
    assert multi == {"size": [104, 60], "mode": 5}  # level 2 of a pyramid: K3p wrote it


def test_chunked_batch(fake_dir):
    text, (r,) = run_case(fake_dir, "e")
    assert r["status"] == [0] * 5 and r["chunks"] == 3
    assert r["sof"] == [list(H.POOL[i][1]) for i in H.CHUNKED_E]
    assert [l.split()[2] for l in text.splitlines() if l.startswith("prep ")] == ["2", "2", "1"]
    # the second and third chunk wait for the other slot's last kernel: an event that has been recorded
    waits = [l for l in text.splitlines() if l.startswith("wait #")]
    assert len(waits) == 2 and "wait #0" not in waits


def test_request_queue_entry_points(fake_dir):
    mem, scaled, fit, multi, bad = run_case(fake_dir, "f")[1]
    assert mem == {"rc": 0, "sof": [64, 64]}
    assert scaled == {"rc": 0, "sof": rule_size((416, 240), scale=1)}
    assert fit == {"rc": 0, "sof": rule_size((480, 272), fit=(100, 0))}
    assert multi["rc"] == 0 and multi["status"] == [0, 0, ERR_OUT_OPTS, 0]
    assert multi["sof"] == [[352, 288], rule_size((352, 288), scale=1), None, rule_size((352, 288), fit=(50, 0))]
    assert bad["rc"] not in (0, ERR_OUT_OPTS) and bad["sof"] is None
