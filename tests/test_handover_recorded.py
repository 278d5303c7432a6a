"""The whole hand-over of the feature cases, against recordings: every case of crop_handover_cases.py,
orient_handover_cases.py, finish_handover_cases.py and rgb_handover_cases.py runs against the stand-in without an
optional stage (tests/fake_gpu/fake_gpu.cpp: `plain`) and against the one with every stage
(tests/fake_gpu/fake_gpu_orient.cpp: `all`), and the child's whole stderr -- the stand-in's transcript and the
`result` lines -- is compared with golden/engine_handover/<module>_<case>_<plain|all>.txt byte for byte (where the two
stand-ins were handed the same bytes, no optional stage being asked for, the one recording <module>_<case>.txt serves both).
A recording is the stderr itself with one abbreviation, undone before the comparison (expanded): the stages of a chunk
get the same descriptor, so a stage line that repeats everything behind the stage's name from the stage line before it is
stored as `<stage> ...`.

The feature tests (test_crop_handover.py, test_orient_handover.py, test_finish_api.py, test_rgb_handover.py) check
chosen lines of these runs; this one checks everything else: the staging digest, every offset, the order of the
event records.  As in test_engine_handover.py the recordings were made once, with the library of the commit before
the host engine was split into modules, and are never regenerated from the code under test: a difference means the
engine now hands the GPU something else, and a missing file fails the test.
"""
import os
import subprocess
import sys

import pytest

from conftest import ROOT, golden
from test_finish_api import IDENT, build_fake

# module -> (its cases, the environment a case's child gets)
MODULES = {
    "crop": ("abcd", {"c": {"H2J_ENGINES": "1"}}),
    "orient": ("abcd", {}),
    "finish": ("abc", {}),
    "rgb": ("abc", {}),
}
STANDINS = {"plain": "fake_gpu.cpp", "all": "fake_gpu_orient.cpp"}
RUNS = [(m, c, s) for m, (cases, _) in sorted(MODULES.items()) for c in cases for s in sorted(STANDINS)]


@pytest.fixture(scope="module")
def lib_dirs(tmp_path_factory):
    return {s: build_fake(tmp_path_factory, "fake_gpu_recorded_" + s, src) for s, src in STANDINS.items()}


def transcript(lib_dir, module, case):
    """The stderr of `python <module>_handover_cases.py <case>` against the stand-in in lib_dir."""
    env = dict(os.environ, H2J_LIB_DIR=lib_dir)
    for k in ("H2J_CHUNK", "H2J_CHUNK_ASYNC", "H2J_ENGINES", "H2J_STRICT_REFERENCE", "H2J_TAIL", "H2J_TAIL_MIN"):
        env.pop(k, None)
    env.update(MODULES[module][1].get(case, {}))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", module + "_handover_cases.py"), case], env=env,
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=120)
    text = p.stderr.decode()
    assert p.returncode == 0, text[-2000:]
    assert text.split("\n", 1)[0] == IDENT, text[:500]
    return text


def expanded(text):
    """The transcript a recording stands for: every `<stage> ...` line with the rest of the stage line before it."""
    out, rest = [], None
    for line in text.split("\n"):
        if line.endswith(" ...") and " " not in line[:-4]:
            assert rest is not None, line
            line = line[:-4] + rest
        elif " nframes " in line:
            rest = line[line.index(" "):]
        out.append(line)
    return "\n".join(out)


def recording(module, case, standin):
    own = golden(os.path.join("engine_handover", f"{module}_{case}_{standin}.txt"))
    return own if os.path.exists(own) else golden(os.path.join("engine_handover", f"{module}_{case}.txt"))


@pytest.mark.parametrize("module,case,standin", RUNS, ids=["-".join(r) for r in RUNS])
def test_transcript_matches_recording(lib_dirs, module, case, standin):
    path = recording(module, case, standin)
    assert os.path.exists(path), f"{path} is missing: recordings come from the commit before the refactor, not from this code"
    with open(path) as f:
        want = expanded(f.read())
    text = transcript(lib_dirs[standin], module, case)
    got_l, want_l = text.splitlines(), want.splitlines()
    first = next((i for i, (a, b) in enumerate(zip(got_l, want_l)) if a != b), min(len(got_l), len(want_l)))
    assert text == want, (f"transcript differs from the recording at line {first + 1}: "
                          f"{got_l[first:first + 1]} vs recorded {want_l[first:first + 1]}")


def test_the_oriented_plans_are_recorded():
    """The new case holds real oriented plans: the all-stages recording shows K3o's map, a pyramid on an oriented
    source and the K3o -> K3u -> K3c chain; the plain one fails those renditions with H2J_ERR_NO_STAGE."""
    with open(recording("orient", "d", "all")) as f:
        lines = expanded(f.read()).splitlines()
    opic = [l for l in lines if l.startswith("opic ")]
    assert sorted({int(l.split()[4]) for l in opic}) == [3, 6, 7]
    assert len(opic) == 6  # P12: 6 (shared by two renditions), 3; P04: 7, 3; A11: 3, 6
    stages = [l.split()[0] for l in lines if " nframes " in l]
    assert stages == ["prep", "predict", "deblock", "sao", "orient", "scale", "finish", "rgb", "jpeg", "entropy"], stages
    with open(recording("orient", "d", "plain")) as f:
        plain = f.read()
    assert "orient map=" not in plain and plain.count("-62") == 8  # the eight oriented renditions of ITEMS_D
