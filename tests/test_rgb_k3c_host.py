"""K3c's lane code on the CPU: csrc/hip/h2j_rgb.hip marks its lane functions __host__ __device__, and
tests/k3c_host/k3c_host.cpp calls them for every lane of 112 outputs -- every source class, layout and store class,
W % 4 == 2 and 2 x 2 among the sizes -- as a stand-alone program whose host code hipcc builds with AddressSanitizer
and UBSan (it starts no kernel and needs no GPU).  A store outside an output's 3 W H bytes (guard bytes round it, the heap block ends behind them), a read
outside the arena or a misaligned 16- / 32-bit store fails the program; its pixels are compared with tests/rgb_ref.py
byte for byte."""
import glob
import os
import subprocess

import numpy as np

import rgb_ref as RGB
from conftest import PKG, ROOT


def test_lane_code_on_the_cpu(tmp_path):
    rocm = os.environ.get("ROCM", "/opt/rocm")
    hipcc = os.environ.get("HIPCC", os.path.join(rocm, "bin", "hipcc"))
    exe = str(tmp_path / "k3c_host")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-x", "hip", "-O1", "-g", "-std=c++17", "-Xarch_host",
                           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(PKG, "csrc", "hip"), os.path.join(ROOT, "tests", "k3c_host", "k3c_host.cpp"),
                           "-o", exe])
    p = subprocess.run([exe, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert p.returncode == 0, p.stdout.decode()[-3000:]
    files = sorted(glob.glob(str(tmp_path / "c*.bin")))
    assert len(files) == 112 and b"112 cases, ok" in p.stdout
    seen = set()
    for fn in files:
        d = np.fromfile(fn, dtype=np.uint8)
        w, h, layout = (int(x) for x in np.frombuffer(d[:12].tobytes(), dtype=np.int32))
        o = 12
        y = d[o:o + w * h].reshape(h, w)
        u = d[o + w * h:o + w * h + w * h // 4].reshape(h // 2, w // 2)
        v = d[o + w * h + w * h // 4:o + w * h + w * h // 2].reshape(h // 2, w // 2)
        got = d[o + w * h + w * h // 2:]
        exp = RGB.convert(y, u, v, "rgb" if layout == 1 else "rgb_planar").reshape(-1)
        assert got.shape == exp.shape and np.array_equal(got, exp), (fn, w, h, layout, np.argwhere(got != exp)[:4].ravel().tolist())
        seen.add((w % 4, layout))
    assert seen == {(0, 1), (0, 2), (2, 1), (2, 2)}
