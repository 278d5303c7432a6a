"""The padded output cases of test_pad_handover.py: what the host engine hands to the GPU library when renditions name
`pad`, in the way handover_cases.py does it (same transcript, a fresh Engine per call).  Run as
`python pad_handover_cases.py <case>` with H2J_LIB_DIR naming the stand-in's directory: case a against
tests/fake_gpu/fake_gpu_orient.cpp, a kernel library with every stage but the padding stage; cases b and c against
tests/fake_gpu/fake_gpu_pad.cpp, which has it.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from handover_cases import P11, P12, P04, A11, BAD, fresh, result, say, stream  # noqa: E402
from rgb_handover_cases import shape_of  # noqa: E402

GREY, RED = (114, 114, 114), (255, 0, 16)

# case a: padded renditions among others, against a kernel library without the stage
ITEMS_A = [
    (P11, [0, {"fit": (90, 70), "pad": True}]),
    (P12, [{"fit": (50, 50), "pad": GREY, "format": "rgb"}]),   # every rendition of the item is padded: the item gets no frame
    (P11, [{"fit": (64, 64), "pad": RED}, {"fit": (65, 65), "pad": True, "format": "rgb"}]),  # nothing to pad: no stage needed
    (A11, [{"pad": True}, 0, {"fit": (80, 80), "pad": True, "scale": 1}]),   # invalid with or without the stage
    (BAD, [{"fit": (90, 70), "pad": True}]),
]

# case b: one fixed chunk.  Views in plan order (frame-major; the unpadded JPEG renditions name theirs first, then the
# padded JPEG renditions their canvases):
#   P12 72 x 40:    0 fit 50 x 26 (K3r; the unpadded JPEG, and the picture part of three padded renditions) |
#                   1 its grey canvas 50 x 50 (a JPEG and a raw rendition) | 2 its black canvas (JPEG)
#   P04 416 x 240:  3 plain (the picture part only: never encoded, 16-bit) | 4 its canvas 500 x 300 (raw only)
#   A11 64 x 64:    5 plain (JPEG) | 6 sharpen 16 (the picture part only: K3u's planes) | 7 its canvas 70 x 66 (JPEG, qscale 7)
ITEMS_B = [
    (P12, [{"fit": (50, 50), "pad": GREY}, {"fit": (50, 50), "pad": GREY, "format": "rgb"}, (50, 50), {"fit": (50, 50), "pad": True}]),
    (P04, [{"fit": (500, 300), "pad": True, "format": "rgb_planar"}]),
    (A11, [{"fit": (70, 66), "pad": RED, "sharpen": 16, "qscale": 7}, 0]),
]

# case c: the largest canvases (include/h2j.h H2J_PAD_MAX_SAMPLES) and the smallest boxes above them
ITEMS_C = [(P11, [{"fit": (8192, 8192), "pad": True}, {"fit": (8194, 8192), "pad": True}, {"fit": (65535, 1025), "pad": GREY},
                  {"cover": (8192, 8194), "pad": True}, {"fit": (65535, 65535), "pad": True}, 0])]


def run(label, items):
    e = fresh()
    say(f"== {label}")
    out = e.transcode_multi([stream(i) for i, _ in items], [r for _, r in items])
    st = e.stats()
    result(status=e.last_status, sof=[[shape_of(j) for j in item] for item in out],
           errors=[e.frame_error(o) for o in range(sum(len(r) for _, r in items))],
           renditions=st["renditions"], parsed=st["parsed"], frames=st["frames"], raw_bytes=st["raw_bytes"], pad_bytes=st["pad_bytes"])


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "h264-h265-to-jpeg_amd"))
    import h2j
    h2j.load_library()  # the stand-in's first transcript line comes before any label
    {"a": lambda: run("without the stage", ITEMS_A), "b": lambda: run("fixed chunk", ITEMS_B), "c": lambda: run("largest canvas", ITEMS_C)}[sys.argv[1]]()
