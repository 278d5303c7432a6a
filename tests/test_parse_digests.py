"""Job records of every golden stream, pinned one by one.

tests/golden/parse_digests.json holds, for every .h264 / .h265 file under tests/golden/, the `parse_bench -r 1 -d`
digest of its job records (transform-block records, coefficients, CTB and slice records, header) as the parser at
commit 25462b4 ("Host engine: options module, one late-stage model, thin C ABI") produced them, or "error" where that
parser refused the stream (tests/golden/malformed).  The branch-miss work on the HEVC slice parser and the Annex-B
scan must leave every one of them as it was.  The parser is built here with the product's compiler
and flags (h264-h265-to-jpeg_amd/Makefile), so that what is pinned is the code the library runs."""
import glob
import json
import os
import shutil
import subprocess

import pytest

from conftest import GOLDEN, PKG, ROOT

PARENT = "25462b4"
HOST = os.path.join(PKG, "csrc", "host")


@pytest.fixture(scope="module")
def parse_bench(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pbd") / "parse_bench")
    rocm = os.environ.get("ROCM", "/opt/rocm")
    clang = os.path.join(rocm, "llvm", "bin", "clang++")
    cxx, tune = (clang, ["-mtune=znver5"]) if os.path.exists(clang) else (shutil.which("g++"), [])
    srcs = [os.path.join(ROOT, "tools", "parse_bench", "parse_bench.cpp")] + [
        os.path.join(HOST, f) for f in ("bitstream.cpp", "cabac_tables.cpp", "hevc_parser.cpp", "h264_parser.cpp")]
    subprocess.check_call([cxx, "-std=c++11", "-O3", "-march=x86-64-v3", "-pthread"] + tune +
                          ["-I", os.path.join(ROOT, "include"), "-I", HOST] + srcs + ["-o", exe])
    return exe


def _streams():
    paths = glob.glob(os.path.join(GOLDEN, "**", "*.h264"), recursive=True) + glob.glob(
        os.path.join(GOLDEN, "**", "*.h265"), recursive=True)
    return sorted(os.path.relpath(p, GOLDEN).replace(os.sep, "/") for p in paths)


def test_every_golden_stream_is_pinned():
    with open(os.path.join(GOLDEN, "parse_digests.json")) as f:
        want = json.load(f)
    assert sorted(want) == _streams()
    assert sum(v != "error" for v in want.values()) >= 250


def test_job_records_equal_the_parent_commits(parse_bench):
    with open(os.path.join(GOLDEN, "parse_digests.json")) as f:
        want = json.load(f)
    got = {}
    for rel in _streams():
        p = subprocess.run([parse_bench, os.path.join(GOLDEN, rel), "-r", "1", "-d"], capture_output=True, text=True)
        got[rel] = p.stdout.split()[-1] if p.returncode == 0 and p.stdout.split() else "error"
    bad = {k: (got[k], want.get(k)) for k in got if got[k] != want.get(k)}
    assert not bad, f"records differ from {PARENT} on {len(bad)} streams: {sorted(bad.items())[:8]}"
