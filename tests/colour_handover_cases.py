"""The colour cases of test_colour_api.py: what the host engine hands to the GPU library when renditions name `colour`,
in the way handover_cases.py does it (same transcript, a fresh Engine per call).  Run as
`python colour_handover_cases.py <case>` with H2J_LIB_DIR naming the directory of the stand-in
tests/fake_gpu/fake_gpu_pad.cpp, a kernel library with every stage but the colour stage.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from handover_cases import P11, P12, P04, A11, BAD, fresh, result, say, stream  # noqa: E402
from rgb_handover_cases import shape_of  # noqa: E402

BT709, JFIF = ("bt709", "limited"), ("bt601", "full")

# case a: converted renditions among others, against a kernel library without the stage
ITEMS_A = [
    (P11, [0, {"fit": (50, 50), "colour": BT709}]),
    (P12, [{"colour": ("bt601", "limited"), "format": "rgb"}]),  # every rendition of the item is converted: the item gets no frame
    (P11, [{"fit": (64, 64), "colour": JFIF}, {"colour": JFIF, "format": "rgb"}, {"colour": "auto", "fit": (32, 32)}]),  # JFIF: no stage needed; auto: bt601 limited
    (A11, [{"colour": BT709, "scale": 7}, 0, {"orient": 6, "colour": BT709, "sharpen": 8}]),
    (BAD, [{"colour": BT709}]),
]

# cases b and c: the same chunk with a colour that resolves to JFIF's, and without the option
ITEMS_B = [
    (P12, [{"fit": (50, 50), "colour": JFIF}, {"fit": (50, 50), "colour": JFIF, "format": "rgb"}, 0]),
    (P04, [{"fit": (500, 300), "pad": True, "colour": JFIF}]),
    (A11, [{"sharpen": 16, "qscale": 7, "colour": JFIF}, {"colour": JFIF}]),
]


def without_colour(items):
    return [(i, [({k: v for k, v in r.items() if k != "colour"} if isinstance(r, dict) else r) for r in rends]) for i, rends in items]


def run(label, items):
    e = fresh()
    say(f"== {label}")
    out = e.transcode_multi([stream(i) for i, _ in items], [r for _, r in items])
    st = e.stats()
    result(status=e.last_status, sof=[[shape_of(j) for j in item] for item in out],
           errors=[e.frame_error(o) for o in range(sum(len(r) for _, r in items))],
           renditions=st["renditions"], parsed=st["parsed"], frames=st["frames"], raw_bytes=st["raw_bytes"], colour_bytes=st["colour_bytes"])


# case v: the validity grid of the word, one item of one rendition per word, through the C calls themselves
VALID = [0, -1] + [0x100 | mc << 1 | f for mc in (1, 5, 6, 9) for f in (0, 1)]
WORDS = sorted(set(VALID + list(range(-4, 40)) + [0x100 | w for w in range(0, 64)] +
                   [0x200, 0x301, 1 << 30, -(1 << 31), (1 << 31) - 1, 0x180, 0x1FF, -0x100]))
WORDS7 = [1, -1, 0x102, 0x10D]  # in the reserved word of h2j_out_opts7


def raw_call(name, otype, field, words):
    import ctypes
    import h2j
    e = fresh()
    n = len(words)
    s = stream(P11)
    bufs = [h2j._u8(s) for _ in range(n)]
    ptrs = (ctypes.POINTER(ctypes.c_uint8) * n)(*bufs)
    sizes = (ctypes.c_size_t * n)(*[len(s)] * n)
    nrend = (ctypes.c_int32 * n)(*[1] * n)
    opts = (otype * n)()
    for o, w in zip(opts, words):
        if field == "colour":
            o.colour = w
        else:
            o.reserved[0] = w
    cap = 1 << 22
    out = (ctypes.c_uint8 * cap)()
    offs, lens, status, wh = (ctypes.c_size_t * n)(), (ctypes.c_size_t * n)(), (ctypes.c_int * n)(), (ctypes.c_int32 * (2 * n))()
    rc = getattr(e._lib, name)(e._h, n, ptrs, sizes, nrend, opts, out, cap, offs, lens, status, wh)
    return rc, list(status), [e.frame_error(i) for i in range(n)]


def case_v():
    import h2j
    say("== the word in h2j_out_opts8")
    rc, st, err = raw_call("h2j_engine_transcode_multi8", h2j.OutOpts8, "colour", WORDS)
    result(rc=rc, status=st, errors=err)
    say("== the word in h2j_out_opts7")
    rc, st, err = raw_call("h2j_engine_transcode_multi7", h2j.OutOpts7, "reserved", WORDS7)
    result(rc=rc, status=st, errors=err)


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "h264-h265-to-jpeg_amd"))
    import h2j
    h2j.load_library()  # the stand-in's first transcript line comes before any label
    {"a": lambda: run("without the stage", ITEMS_A), "b": lambda: run("fixed chunk", ITEMS_B),
     "c": lambda: run("fixed chunk", without_colour(ITEMS_B)), "v": case_v}[sys.argv[1]]()
