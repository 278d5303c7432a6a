"""K3v's lane code on the CPU: csrc/hip/h2j_colour.hip marks its lane functions __host__ __device__, and
tests/k3v_host/k3v_host.cpp calls them for every lane of 504 outputs -- every source class and both work classes, all six
constant sets, W % 8 = 0, 2, 4, 6, a single chroma row and 2 x 2 among the sizes -- as a stand-alone program whose host
code hipcc builds with AddressSanitizer and UBSan (it starts no kernel and needs no GPU).  A store outside an output's
planes (guard bytes round them, the heap block ends behind them), a read outside the arena or a misaligned 32-bit access
fails the program; its planes are compared with tests/colour_ref.py byte for byte."""
import glob
import os
import subprocess

import numpy as np

import colour_ref as COL
from conftest import PKG, ROOT


def test_lane_code_on_the_cpu(tmp_path):
    rocm = os.environ.get("ROCM", "/opt/rocm")
    hipcc = os.environ.get("HIPCC", os.path.join(rocm, "bin", "hipcc"))
    exe = str(tmp_path / "k3v_host")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-x", "hip", "-O1", "-g", "-std=c++17", "-Xarch_host",
                           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(PKG, "csrc", "hip"), os.path.join(ROOT, "tests", "k3v_host", "k3v_host.cpp"),
                           "-o", exe])
    p = subprocess.run([exe, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert p.returncode == 0, p.stdout.decode()[-3000:]
    files = sorted(glob.glob(str(tmp_path / "c*.bin")))
    assert len(files) == 504 and b"504 cases, ok" in p.stdout
    seen, clips = set(), set()
    for fn in files:
        d = np.fromfile(fn, dtype=np.uint8)
        w, h, mc, full = (int(x) for x in np.frombuffer(d[:16].tobytes(), dtype=np.int32))
        n = w * h * 3 // 2
        assert d.size == 16 + 2 * n, (fn, d.size)

        def planes(a):
            return a[:w * h].reshape(h, w), a[w * h:w * h + w * h // 4].reshape(h // 2, w // 2), a[w * h + w * h // 4:].reshape(h // 2, w // 2)

        y, u, v = planes(d[16:16 + n])
        got = planes(d[16 + n:])
        matrix, rng = COL.MC_NAME[mc], "full" if full else "limited"
        exp = COL.convert(y, u, v, matrix, rng)
        for name, g, e in zip("YUV", got, exp):
            assert np.array_equal(g, e), (fn, w, h, matrix, rng, name, np.argwhere(g != e)[:4].ravel().tolist())
        seen.add((w % 8, mc, full))
        for name, s, sh in zip("YUV", COL.sums(y, u, v, matrix, rng), (20, 16, 16)):
            if int(s.min()) < 0:
                clips.add(name + "lo")
            if int(s.max()) >> sh > 255:
                clips.add(name + "hi")
    assert {m for m, _, _ in seen} == {0, 2, 4, 6} and {(mc, f) for _, mc, f in seen} == {(6, 0), (6, 1), (1, 0), (1, 1), (9, 0), (9, 1)}
    assert clips == {"Ylo", "Yhi", "Ulo", "Uhi", "Vlo", "Vhi"}, clips
