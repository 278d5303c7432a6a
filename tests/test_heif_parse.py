"""HEIF input through the entropy decoders: job records, pinned by the digests of tools/parse_bench (the tool
test_parse_digests.py uses), built here with -DH2J_HEIF_INPUT and the two HEIF sources beside the parsers.

A single-item HEIC must parse to the records of the Annex-B stream it wraps.  A grid parses to one canvas picture
whose records do not depend on the thread count.  hevcgen cannot write the real tiled stream that would equal set b's
canvas: its mode and SAO choices draw from one random sequence across the whole picture, so the tiles of a tiled
picture are not the pictures it codes one by one from the same content; that equality stays unchecked on the CPU, and
the GPU suite (test_gpu_heif.py) checks the canvas against the oracle's decode of every tile instead."""
import json
import os
import shutil
import subprocess

import pytest

import heif_mux as M
import heif_ref as HR
from conftest import GOLDEN, PKG, ROOT, golden, read

HOST = os.path.join(PKG, "csrc", "host")


@pytest.fixture(scope="module")
def parse_bench(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pbh") / "parse_bench")
    rocm = os.environ.get("ROCM", "/opt/rocm")
    clang = os.path.join(rocm, "llvm", "bin", "clang++")
    cxx, tune = (clang, ["-mtune=znver5"]) if os.path.exists(clang) else (shutil.which("g++"), [])
    srcs = [os.path.join(ROOT, "tools", "parse_bench", "parse_bench.cpp")] + [
        os.path.join(HOST, f) for f in ("bitstream.cpp", "cabac_tables.cpp", "hevc_parser.cpp", "h264_parser.cpp", "heif.cpp", "heif_parse.cpp")]
    subprocess.check_call([cxx, "-std=c++11", "-O3", "-march=x86-64-v3", "-pthread", "-DH2J_HEIF_INPUT"] + tune +
                          ["-I", os.path.join(ROOT, "include"), "-I", HOST] + srcs + ["-o", exe])
    return exe


def digest(exe, tmp, data, threads=1):
    """(digest, None) or (None, the parser's message)"""
    path = str(tmp / "in.bin")
    with open(path, "wb") as f:
        f.write(data)
    p = subprocess.run([exe, path, "-r", "1", "-d", "-p", str(threads)], capture_output=True, text=True)
    if p.returncode == 0 and p.stdout.split():
        return p.stdout.split()[-1], None
    return None, p.stderr.strip()


def test_single_items_parse_to_their_streams_records(parse_bench, tmp_path):
    with open(os.path.join(GOLDEN, "parse_digests.json")) as f:
        pinned = json.load(f)
    for name, codec in (("img01.h265", 265), ("img01.h264", 264), ("hevc/p11_64x64_tiny.h265", 265),
                        ("hevc/p18_416x240_tiles3x2_ctb32.h265", 265), ("h264/a11_64x64_tiny.h264", 264)):
        s = read(golden(name))
        for k in ({}, dict(iloc_version=1, construction=1, extents=3, mdat_first=True)):
            assert digest(parse_bench, tmp_path, M.mux([s], codec=codec, **k)) == (pinned[name], None), name
        assert digest(parse_bench, tmp_path, s) == (pinned[name], None)


@pytest.mark.parametrize("case", HR.CASES, ids=lambda c: f"{c[0]}_{c[1]}x{c[2]}")
def test_grid_records_do_not_depend_on_threads(parse_bench, tmp_path, case):
    name, cols, rows, W, H = case
    data = M.mux(list(HR.tiles(name))[:rows * cols], grid=(rows, cols, W, H))
    one = digest(parse_bench, tmp_path, data, 1)
    assert one[0] and one[1] is None, one
    assert digest(parse_bench, tmp_path, data, 8) == one
    assert digest(parse_bench, tmp_path, data, 3) == one


def test_one_tile_grid_is_the_picture(parse_bench, tmp_path):
    """a 1 x 1 grid whose output is the tile: the records of the tile picture itself"""
    s = HR.tiles("e")[0]
    assert digest(parse_bench, tmp_path, M.mux([s], grid=(1, 1, 256, 256))) == digest(parse_bench, tmp_path, s)


def test_grid_rejections(parse_bench, tmp_path):
    a, b = HR.tiles("a"), HR.tiles("b")
    p09 = read(golden("hevc/p09_200x120_noqpd_notskip.h265"))  # 200 x 120 coded: no CTB multiple
    p15 = read(golden("hevc/p15_48x200_wpp_narrow.h265"))
    a1_pps = read(golden("heif/a_1_pps.hevc"))
    sets = lambda s: [[n for n in M.split_nals(s) if (n[0] >> 1) & 63 == t] for t in (33, 34)]
    assert sets(a1_pps)[0] == sets(a[1])[0] and sets(a1_pps)[1] != sets(a[1])[1]  # what the vector is for
    cases = [
        (M.mux([a[0], b[1], a[2], a[3]], grid=(2, 2, 128, 128)), "HEIF grid: tiles carry different SPS"),  # CTB 16 / 64
        # tile 1 coded once more with another pps_cb_qp_offset: the same SPS bytes, another PPS
        (M.mux([a[0], a1_pps, a[2], a[3]], grid=(2, 2, 128, 128)), "HEIF grid: tiles carry different PPS"),
        (M.mux([a1_pps, a[1], a[2], a[3]], grid=(2, 2, 128, 128)), "HEIF grid: tiles carry different PPS"),
        (M.mux([p09, p09], grid=(1, 2, 400, 120)), "HEIF grid: tile size is not a multiple of the CTB size"),
        (M.mux([p15, p15], grid=(1, 2, 96, 200)), "HEIF grid: a tile picture uses tiles or wavefront parallel processing"),
        (M.mux(list(HR.tiles("h264")), grid=(2, 2, 128, 128), tile_codec=264), "HEIF: grid of AVC tiles unsupported"),
        (M.mux(list(a), grid=(2, 2, 64, 100)), "HEIF grid: output size does not end in the last tile row and column"),
        (M.mux(list(a), grid=(2, 2, 130, 100)), "HEIF grid: output size does not end in the last tile row and column"),
        # legal by the grid's rule (W > (cols - 1) tw), but rounded down to even nothing of the last column is left
        (M.mux(list(a), grid=(2, 2, 65, 100)), "HEIF grid: odd output size one sample past a tile border is unsupported"),
        (M.mux(list(a), grid=(2, 2, 100, 65)), "HEIF grid: odd output size one sample past a tile border is unsupported"),
    ]
    for data, message in cases:
        d, err = digest(parse_bench, tmp_path, data)
        assert d is None and err.endswith(message), (err, message)
