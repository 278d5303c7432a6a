"""K3b's lane code on the CPU: csrc/hip/h2j_pad.hip marks its lane functions __host__ __device__, and
tests/k3b_host/k3b_host.cpp calls them for every thread of every workgroup of 124 records -- the placements of
tests/test_gpu_pad.py and every p & 3 of the luma and the chroma, in every source class -- as a stand-alone program whose
host code hipcc builds with AddressSanitizer and UBSan (it starts no kernel and needs no GPU).  A load outside the source
planes (a heap block of exactly their bytes), a store outside the canvas (a block of its own, guard bytes round it), a
byte of the canvas's rows left unwritten or a misaligned 32-bit access fails the program; its canvases are compared with tests/pad_ref.py byte
for byte."""
import glob
import os
import subprocess

import numpy as np

import pad_ref as PAD
from conftest import PKG, ROOT


def test_lane_code_on_the_cpu(tmp_path):
    rocm = os.environ.get("ROCM", "/opt/rocm")
    hipcc = os.environ.get("HIPCC", os.path.join(rocm, "bin", "hipcc"))
    exe = str(tmp_path / "k3b_host")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-x", "hip", "-O1", "-g", "-std=c++17", "-Xarch_host",
                           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(PKG, "csrc", "hip"), os.path.join(ROOT, "tests", "k3b_host", "k3b_host.cpp"),
                           "-o", exe])
    p = subprocess.run([exe, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert p.returncode == 0, p.stdout.decode()[-3000:]
    files = sorted(glob.glob(str(tmp_path / "c*.bin")))
    assert len(files) == 124 and b"124 cases, ok" in p.stdout
    shifts = set()
    for fn in files:
        d = np.fromfile(fn, dtype=np.uint8)
        w, h, bw, bh, px, py, fy, fu, fv = (int(x) for x in np.frombuffer(d[:36].tobytes(), dtype=np.int32))
        o = 36

        def take(rows, cols):
            nonlocal o
            a = d[o:o + rows * cols].reshape(rows, cols)
            o += rows * cols
            return a

        y, u, v = take(h, w), take(h // 2, w // 2), take(h // 2, w // 2)
        got = take(bh, bw), take(bh // 2, bw // 2), take(bh // 2, bw // 2)
        assert o == d.size
        exp = PAD.pad_planes(y, u, v, bw, bh, px, py, (fy, fu, fv))
        for c in range(3):
            assert np.array_equal(got[c], exp[c]), (fn, (w, h, bw, bh, px, py), c, np.argwhere(got[c] != exp[c])[:4].tolist())
        shifts.add((px & 3, (px >> 1) & 3))
    assert shifts == {(0, 0), (2, 1), (0, 2), (2, 3)}
