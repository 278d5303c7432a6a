"""The RGB output cases of test_rgb_handover.py: what the host engine hands to the GPU library when renditions name
a format, in the way handover_cases.py does it (same transcript, a fresh Engine per call).  Run as
`python rgb_handover_cases.py <case>` with H2J_LIB_DIR naming the stand-in's directory: case a against
tests/fake_gpu/fake_gpu.cpp, a kernel library without the RGB stage; cases b and c against
tests/fake_gpu/fake_gpu_rgb.cpp, which has it.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from handover_cases import P11, P12, P04, A11, BAD, fresh, result, say, sof_size, stream  # noqa: E402

# case a: raw renditions among plain items, against a kernel library without the stage
ITEMS_A = [
    (P11, [0, {"format": "rgb"}]),
    (P04, [{"scale": 1, "format": "rgb_planar"}, 1]),
    (BAD, [{"format": "rgb"}]),
    (A11, [{"format": "rgb", "qscale": 9}, 0]),   # invalid with or without the stage
    (P12, [{"format": "rgb"}]),   # every rendition of the item is raw: the item gets no frame
]

# case b: one fixed chunk.  Views in plan order (frame-major, the plain unscaled view of a frame first; the JPEG
# renditions name theirs before the raw ones look for one):
#   P12 72 x 40:    0 plain (JPEG, and the planar raw output) | 1 scale 1 (JPEG, and the raw output) | 2 scale 1 qscale 7
#   P04 416 x 240:  3 scale 2 sharpen 16 (raw only: a view of its own, K3u's planes) | 4 crop, unscaled (raw only, 16-bit)
#   A11 64 x 64:    5 plain (raw only, both layouts)
ITEMS_B = [
    (P12, [{"scale": 1, "format": "rgb"}, 1, {"scale": 1, "qscale": 7}, {"format": "rgb_planar"}, 0, {"scale": 1, "format": "rgb"}]),
    (P04, [{"scale": 2, "sharpen": 16, "format": "rgb"}, {"crop": (36, 10, 300, 200), "format": "rgb_planar"}]),
    (A11, [{"format": "rgb"}, {"format": "rgb_planar"}]),
]
# the K3c map by class: wide, 8-bit, 16-bit (view-major inside a class)
PX_B = ["px 36 20 layout 1 depth 8,8 wide 1 crop 0,0 pitch 48,32,32 base 0 at 0 own 1",
        "px 104 60 layout 1 depth 8,8 wide 1 crop 0,0 pitch 112,64,64 base 0 at 0 own 1",
        "px 72 40 layout 2 depth 8,8 wide 0 crop 0,0 pitch 72,36,36 base 0 at 0 own 1",
        "px 64 64 layout 1 depth 8,8 wide 0 crop 0,0 pitch 64,32,32 base 0 at 0 own 1",
        "px 64 64 layout 2 depth 8,8 wide 0 crop 0,0 pitch 64,32,32 base 0 at 0 own 1",
        "px 300 200 layout 2 depth 10,10 wide 0 crop 36,10 pitch 416,208,208 base 0 at 0 own 1"]


# case c: a chunk of raw renditions only -- the input-pipeline call: no K4 / K5, no payload copy
ITEMS_C = [(P11, [{"fit": (32, 32), "format": "rgb"}]), (P12, [{"format": "rgb_planar"}, {"format": "rgb"}])]


def shape_of(o):
    if isinstance(o, np.ndarray):
        return ["px"] + list(o.shape)
    return sof_size(o)


def run(label, items):
    e = fresh()
    say(f"== {label}")
    out = e.transcode_multi([stream(i) for i, _ in items], [r for _, r in items])
    result(status=e.last_status, sof=[[shape_of(j) for j in item] for item in out],
           errors=[e.frame_error(o) for o in range(sum(len(r) for _, r in items))],
           renditions=e.stats()["renditions"], parsed=e.stats()["parsed"], frames=e.stats()["frames"], raw_bytes=e.stats()["raw_bytes"])


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "h264-h265-to-jpeg_amd"))
    import h2j
    h2j.load_library()  # the stand-in's first transcript line comes before any label
    {"a": lambda: run("without the stage", ITEMS_A), "b": lambda: run("fixed chunk", ITEMS_B), "c": lambda: run("raw only", ITEMS_C)}[sys.argv[1]]()
