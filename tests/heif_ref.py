"""The picture a HEIF grid shows, from the oracle alone (test infrastructure).

ISO/IEC 23008-12 6.6.2.3: the reconstructed image of a grid item is the tile images, each decoded on its own, placed
side by side in raster order without overlap, and cropped on the right and at the bottom to output_width x
output_height.  Each tile is decoded here by the CPU oracle (oracle_py) as the whole picture it is; nothing of the
product's canvas construction is used.  An odd output size rounds down to even, as the product documents it (a 4:2:0
conformance window cannot express an odd size)."""
import functools
import json
import os

import numpy as np

import oracle_py as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "heif")

# set -> [(cols, rows, W, H)]: the grids the suites build from each tile set (tools/make_streams.py heif)
GRIDS = {
    "a": [(2, 2, 120, 100)],
    "b": [(3, 2, 192, 128)],
    "c": [(1, 3, 64, 96), (3, 1, 192, 32)],
    "d": [(2, 2, 256, 256)],
    "e": [(3, 2, 700, 500)],
}
CASES = [(name,) + g for name in sorted(GRIDS) for g in GRIDS[name]]


@functools.lru_cache(maxsize=None)
def manifest():
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        return {m["set"]: m for m in json.load(f)}


@functools.lru_cache(maxsize=None)
def tiles(name):
    """the set's tile streams in raster order"""
    ext = "avc" if name == "h264" else "hevc"
    out = []
    for t in range(manifest()[name]["tiles"]):
        with open(os.path.join(GOLDEN, f"{name}_{t}.{ext}"), "rb") as f:
            out.append(f.read())
    return tuple(out)


@functools.lru_cache(maxsize=None)
def canvas(name, cols, rows, W, H):
    """(Y, U, V uint16, bit depth) of the grid: oracle-decoded tiles composed and cropped.  Read-only arrays."""
    dec = [O.decode(s, 265) for s in tiles(name)[:cols * rows]]
    bd = dec[0][3]
    planes = []
    for c in range(3):
        planes.append(np.concatenate([np.concatenate([dec[r * cols + k][c] for k in range(cols)], axis=1) for r in range(rows)], axis=0))
    W2, H2 = W & ~1, H & ~1
    out = [planes[0][:H2, :W2].copy(), planes[1][:H2 // 2, :W2 // 2].copy(), planes[2][:H2 // 2, :W2 // 2].copy()]
    for p in out:
        p.setflags(write=False)
    return out[0], out[1], out[2], bd
