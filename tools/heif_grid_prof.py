"""Phone-size HEIF grid: the lone-picture parse time with 1 and 16 threads, beside one Annex-B picture of the canvas
size (profiles/heif_grid.md).  Nothing it mints is committed.

  python tools/heif_grid_prof.py mint DIR     48 tiles of 512 x 512 (8 x 6 -> 4032 x 3024) and the 4096 x 3072 canvas
                                              content as one picture, encoded by tools/hevcgen into DIR
  python tools/heif_grid_prof.py time DIR     build tools/parse_bench with HEIF input, time both inputs with
                                              -p 1 and -p 16, print a markdown table
  python tools/heif_grid_prof.py gpu DIR      decode the grid on the GPU and compare it with the oracle's decode of
                                              every tile, composed and cropped; time transcode of the lone file
"""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "h264-h265-to-jpeg_amd"))

COLS, ROWS, TW, TH, W, H, QP = 8, 6, 512, 512, 4032, 3024, 26


def mint(d):
    import make_streams as MS
    import heif_mux as M
    MS.build_gen()
    os.makedirs(d, exist_ok=True)
    canvas = MS.make_content(MS.source_planes(), COLS * TW, ROWS * TH, 4800, 3, 8, upsample=3)
    tiles = []
    for t in range(COLS * ROWS):
        ty, tx = divmod(t, COLS)
        tile = [canvas[0][ty * TH:(ty + 1) * TH, tx * TW:(tx + 1) * TW]] + [
            p[ty * TH // 2:(ty + 1) * TH // 2, tx * TW // 2:(tx + 1) * TW // 2] for p in canvas[1:]]
        path = os.path.join(d, f"tile_{t:02d}.hevc")
        MS.encode(tile, TW, TH, 8, QP, 4800 + t, path, ["--ctb", "64", "--sao", "1"])
        tiles.append(open(path, "rb").read())
    nb = MS.encode(canvas, COLS * TW, ROWS * TH, 8, QP, 4900, os.path.join(d, "canvas.h265"), ["--ctb", "64", "--sao", "1"])
    heic = M.mux(tiles, grid=(ROWS, COLS, W, H), tile_size=(TW, TH))
    with open(os.path.join(d, "grid.heic"), "wb") as f:
        f.write(heic)
    print(f"grid.heic {len(heic)} B ({COLS * ROWS} tiles), canvas.h265 {nb} B")


def timings(d):
    host = os.path.join(ROOT, "h264-h265-to-jpeg_amd", "csrc", "host")
    exe = os.path.join(d, "parse_bench_heif")
    clang = os.path.join(os.environ.get("ROCM", "/opt/rocm"), "llvm", "bin", "clang++")
    cxx, tune = (clang, ["-mtune=znver5"]) if os.path.exists(clang) else ("g++", [])
    srcs = [os.path.join(ROOT, "tools", "parse_bench", "parse_bench.cpp")] + [
        os.path.join(host, f) for f in ("bitstream.cpp", "cabac_tables.cpp", "hevc_parser.cpp", "h264_parser.cpp", "heif.cpp", "heif_parse.cpp")]
    subprocess.check_call([cxx, "-std=c++11", "-O3", "-march=x86-64-v3", "-pthread", "-DH2J_HEIF_INPUT"] + tune +
                          ["-I", os.path.join(ROOT, "include"), "-I", host] + srcs + ["-o", exe])
    print("| input | bytes | threads | ms per picture (best of 5 runs of 8) | digest |")
    print("|---|---|---|---|---|")
    for name in ("grid.heic", "canvas.h265"):
        path = os.path.join(d, name)
        for p in (1, 16):
            best, dig = 1e9, ""
            for _ in range(5):
                w = subprocess.check_output([exe, path, "-r", "8", "-t", "1", "-p", str(p), "-d"], text=True).split()
                best, dig = min(best, float(w[2])), w[-1]
            print(f"| {name} | {os.path.getsize(path)} | {p} | {best:.2f} | {dig} |", flush=True)


def gpu(d):
    import h2j
    import heif_mux as M
    import oracle_py as O
    tiles = [open(os.path.join(d, f"tile_{t:02d}.hevc"), "rb").read() for t in range(COLS * ROWS)]
    heic = open(os.path.join(d, "grid.heic"), "rb").read()
    assert heic == M.mux(tiles, grid=(ROWS, COLS, W, H), tile_size=(TW, TH))
    dec = [O.decode(s, 265) for s in tiles]
    want = [np.concatenate([np.concatenate([dec[r * COLS + c][k] for c in range(COLS)], axis=1) for r in range(ROWS)], axis=0)
            for k in range(3)]
    e = h2j.Engine()
    y, u, v, bd = e.decode(heic)
    ok = (np.array_equal(y, want[0][:H, :W]) and np.array_equal(u, want[1][:H // 2, :W // 2]) and np.array_equal(v, want[2][:H // 2, :W // 2]))
    print(f"grid planes {y.shape[1]} x {y.shape[0]} vs the oracle's tiles composed: {'bit-exact' if ok else 'DIFFERENT'}")
    for name, data in (("grid.heic", heic), ("canvas.h265", open(os.path.join(d, "canvas.h265"), "rb").read())):
        e.transcode([data])
        best = 1e9
        for _ in range(8):
            t0 = time.perf_counter()
            (out,) = e.transcode([data])
            best = min(best, time.perf_counter() - t0)
        print(f"transcode of the lone {name}: {best * 1e3:.2f} ms (best of 8), JPEG {len(out)} B")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit({"mint": mint, "time": timings, "gpu": gpu}[sys.argv[1]](sys.argv[2]) or 0)
