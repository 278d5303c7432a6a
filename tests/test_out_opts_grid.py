"""The output-options rule against golden/out_opts/grid.txt (tests/out_opts_grid.py says what a line is), two ways:
through the built libH265ToJpeg.so, loaded by a child python beside a stand-in kernel library, and through the
stand-alone program tests/out_opts_host/out_opts_host.cpp, which links csrc/host/out_opts.cpp and nothing else of
the project and runs under AddressSanitizer and UBSan.  Both must print the recording byte for byte.  The recording
comes from the commit before the options moved into their module; a missing file fails the test."""
import os
import subprocess
import sys

import out_opts_grid as G
from conftest import PKG, ROOT, golden
from test_finish_api import build_fake


def recorded():
    path = golden(os.path.join("out_opts", "grid.txt"))
    assert os.path.exists(path), f"{path} is missing: the recording comes from the commit before the refactor"
    with open(path) as f:
        return path, f.read()


def first_difference(got, want):
    g, w = got.splitlines(), want.splitlines()
    i = next((i for i, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
    return f"line {i + 1}: {g[i:i + 1]} vs recorded {w[i:i + 1]}"


def test_grid_holds_the_calls():
    _, want = recorded()
    lines = want.splitlines()
    assert [l.split(" -> ")[0] for l in lines] == G.calls() and len(lines) < 5000
    ok = sum(l.split(" -> ")[1].startswith("0 ") for l in lines)
    assert 300 < ok < len(lines) - 300  # both accepted and refused option sets, plenty of each


def test_library_answers_the_grid(tmp_path_factory):
    _, want = recorded()
    d = build_fake(tmp_path_factory, "fake_gpu_grid", "fake_gpu.cpp")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "out_opts_grid.py")], env=dict(os.environ, H2J_LIB_DIR=d),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    got = p.stdout.decode()
    assert got == want, first_difference(got, want)


def test_module_alone_answers_the_grid(tmp_path):
    path, want = recorded()
    exe = str(tmp_path / "out_opts_host")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++11", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "csrc", "host"),
                           os.path.join(ROOT, "tests", "out_opts_host", "out_opts_host.cpp"), os.path.join(PKG, "csrc", "host", "out_opts.cpp"),
                           "-o", exe])
    p = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0 and not p.stderr, p.stderr.decode()[-3000:]
    got = p.stdout.decode()
    assert got == want, first_difference(got, want)
