"""The crop and cover cases of test_crop_handover.py: what the host engine hands to the GPU library for
windowed renditions, in the way handover_cases.py does it (same stand-in, same transcript, a fresh Engine
per call).  Run as `python crop_handover_cases.py <case>` with H2J_LIB_DIR naming the stand-in's directory.
"""
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from handover_cases import POOL, P11, P12, P04, P19, A04, A11, A31, BAD, fresh, result, say, sof_size, stream  # noqa: E402

# case a: per-item rendition lists (streams by POOL index)
ITEMS_A = [
    (P11, [{"crop": (16, 16, 32, 32)}, {"crop": (2, 2, 2, 2)}, 0, {"crop": (0, 0, 64, 64)}]),
    (P04, [{"crop": (36, 10, 300, 200), "scale": 1}, {"crop": (36, 10, 300, 200), "scale": 2},
           {"crop": (36, 10, 300, 200), "scale": 3}, {"crop": (6, 4, 250, 150), "fit": (100, 0)},
           {"cover": (64, 64)}, {"crop": (100, 0, 0, 0), "cover": (50, 100)}]),
    (P19, [{"cover": (480, 272)}, {"cover": (120, 68)}, {"crop": (0, 0, 0, 0), "max_dim": 100}]),
    # invalid renditions between valid ones: odd x, odd w, x + w > W, h resolving to 0, a negative field,
    # cover with stretch, cover with fit_h 0, cover with a scale
    (A04, [{"crop": (3, 0, 0, 0)}, 1, {"crop": (0, 0, 33, 32)}, {"crop": (300, 0, 64, 32)}, {"crop": (0, 288, 0, 0)},
           {"crop": (-2, 0, 0, 0)}, {"cover": (16, 16), "stretch": True}, {"crop": (32, 32, 64, 64)}]),
    (A31, [{"cover": (16, 0)}, {"cover": (16, 16), "scale": 1}, {"cover": (16, 16)}]),
    (BAD, [{"crop": (0, 0, 16, 16)}, 0]),
    (P12, [{"crop": (2, 2, 60, 30), "scale": 1}]),
]

# case b: the same call with and without windows that resolve to the whole picture
SAME_B = [
    ([P11, P04, A04], [[0], [1, 2], [(50, 0)]],
     [[{"crop": (0, 0, 64, 64)}], [{"crop": (0, 0, 0, 0), "scale": 1}, {"crop": (0, 0, 416, 240), "scale": 2}],
      [{"crop": (0, 0, 352, 0), "fit": (50, 0)}]]),
    ([P19], [[(120, 68)]], [[{"cover": (120, 68)}]]),  # the box has the picture's aspect: the fit, byte for byte
]


def case_a():
    e = fresh()
    say("== transcode_multi, windows")
    out = e.transcode_multi([stream(i) for i, _ in ITEMS_A], [r for _, r in ITEMS_A])
    result(status=e.last_status, sof=[[sof_size(j) for j in item] for item in out],
           errors=[e.frame_error(o) for o in range(sum(len(r) for _, r in ITEMS_A))],
           renditions=e.stats()["renditions"], parsed=e.stats()["parsed"])


def case_b():
    for k, (idx, plain, windowed) in enumerate(SAME_B):
        for label, rend in (("plain", plain), ("window", windowed)):
            e = fresh()
            say(f"== {k} {label}")
            out = e.transcode_multi([stream(i) for i in idx], rend)
            result(status=e.last_status, sof=[[sof_size(j) for j in item] for item in out])


def case_c():
    import h2j
    lib = h2j.load_library()
    u8p = ctypes.POINTER(ctypes.c_uint8)
    say("== h2j_h265_to_jpeg_mem_multi3")
    s = stream(P04)
    specs = [{"crop": (36, 10, 300, 200)}, {"cover": (64, 64)}, {"crop": (1, 0, 0, 0)}, 1]
    n = len(specs)
    opts = (h2j.OutOpts3 * n)(*[h2j.OutOpts3(*(h2j.rendition_spec(x) + (0, 0, 0, 0))[:9]) for x in specs])
    jp, ln, st = (u8p * n)(), (ctypes.c_size_t * n)(), (ctypes.c_int * n)()
    rc = lib.h2j_h265_to_jpeg_mem_multi3(h2j._u8(s), len(s), n, opts, jp, ln, st)
    sof = []
    for r in range(n):
        sof.append(sof_size(ctypes.string_at(jp[r], ln[r])) if st[r] == 0 else None)
        if jp[r]:
            lib.h2j_free(ctypes.cast(jp[r], ctypes.c_void_p))
    result(rc=rc, status=list(st), sof=sof)
    say("== decode_multi3")
    y, u, v, size, mode, win = fresh().decode_multi3(s, [{"crop": (36, 10, 300, 200), "scale": 1},
                                                         {"crop": (36, 10, 300, 200), "scale": 2}, 1], 1)
    result(size=list(size), mode=mode, window=list(win), shape=list(y.shape))


# case d: items whose every rendition fails only once the picture's size is known (the window lies outside
# it): such an item is parsed and gets no frame in the chunk
OUTSIDE = (100, 0, 32, 32)  # of a 64 x 64 picture
CALLS_D = [
    ([P11], [[{"crop": OUTSIDE}]]),                                                      # alone
    ([P04, P11, A04], [[0], [{"crop": OUTSIDE}], [1]]),                                  # between good items
    ([P11, P12], [[{"crop": OUTSIDE}, {"crop": (0, 80, 0, 0), "scale": 1}, {"crop": (60, 60, 8, 8), "fit": (2, 2)}],
                  [{"crop": (2, 2, 60, 30), "scale": 1}]]),                              # every rendition of an item
    ([P11, A11], [[{"crop": OUTSIDE}], [{"crop": (0, 0, 0, 66)}]]),                      # no frame at all in the batch
]


def case_d():
    for k, (idx, rend) in enumerate(CALLS_D):
        e = fresh()
        say(f"== {k} windows outside the picture")
        out = e.transcode_multi([stream(i) for i in idx], rend)
        st = e.stats()
        result(status=e.last_status, sof=[[sof_size(j) for j in item] for item in out],
               errors=[e.frame_error(o) for o in range(sum(len(r) for r in rend))],
               frames=st["frames"], renditions=st["renditions"], parsed=st["parsed"])
    e = fresh()
    say("== keyword form")
    out = e.transcode([stream(P11), stream(P12)], crop=[OUTSIDE, None])
    result(status=e.last_status, sof=[sof_size(j) for j in out])


CASES = {"a": case_a, "b": case_b, "c": case_c, "d": case_d}
ENV = {"c": {"H2J_ENGINES": "1"}}

if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "h264-h265-to-jpeg_amd"))
    import h2j
    h2j.load_library()
    CASES[sys.argv[1]]()
