"""The orientation cases of test_orient_handover.py: what the host engine hands to the GPU library when
renditions carry an orientation, in the way handover_cases.py does it (same stand-in, same transcript, a
fresh Engine per call).  The stand-in has no h2j_gpu_orient: it is the older kernel library of the
H2J_ERR_NO_STAGE rule (test_handover_recorded.py also runs every case, case d for its oriented plans, against
tests/fake_gpu/fake_gpu_orient.cpp, which has the stage).  Run as `python orient_handover_cases.py <case>` with H2J_LIB_DIR naming the
stand-in's directory.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from handover_cases import POOL, P11, P12, P04, P19, A04, A11, A31, BAD, fresh, result, say, sof_size, stream  # noqa: E402
import orient_ref as O  # noqa: E402

# case a: the same call through the multi3 / multi call and through multi4 with orientations that resolve to 0
SAME_A = [
    ([P11, P04, A04], [[0], [1, 2, {"crop": (36, 10, 300, 200)}], [{"cover": (64, 64)}, (50, 0)]],
     [[{"orient": 0}], [{"orient": 1, "scale": 1}, {"orient": 0, "scale": 2}, {"orient": 1, "crop": (36, 10, 300, 200)}],
      [{"orient": 0, "cover": (64, 64)}, {"orient": 0, "fit": (50, 0)}]]),
    # auto on streams without the SEI
    ([P12, P19, A31], [[0, 1], [{"crop": (16, 16, 64, 64)}], [0]],
     [[{"orient": "auto"}, {"orient": "auto", "scale": 1}], [{"orient": "auto", "crop": (16, 16, 64, 64)}], [{"orient": "auto"}]]),
]

# case b: one oriented rendition among plain items, against a kernel library without the stage
ITEMS_B = [
    (P11, [0, 1]),
    (P04, [0, {"orient": 6}, {"crop": (36, 10, 300, 200), "scale": 1}]),
    (BAD, [0]),
    (A04, [{"orient": 9}, 1]),
    (P12, [{"orient": 3, "scale": 1}]),   # every rendition of the item is oriented: the item gets no frame
]


def without_oriented(specs):
    return [s for s in specs if not (isinstance(s, dict) and 2 <= s.get("orient", 0) <= 8)]


def case_a():
    for k, (idx, plain, oriented) in enumerate(SAME_A):
        for label, rend in (("plain", plain), ("orient", oriented)):
            e = fresh()
            say(f"== {k} {label}")
            out = e.transcode_multi([stream(i) for i in idx], rend)
            result(status=e.last_status, sof=[[sof_size(j) for j in item] for item in out])


def case_b():
    for label, items in (("with", ITEMS_B), ("without", [(i, without_oriented(r)) for i, r in ITEMS_B if without_oriented(r)])):
        e = fresh()
        say(f"== {label} the oriented renditions")
        out = e.transcode_multi([stream(i) for i, _ in items], [r for _, r in items])
        result(status=e.last_status, sof=[[sof_size(j) for j in item] for item in out],
               errors=[e.frame_error(o) for o in range(sum(len(r) for _, r in items))],
               renditions=e.stats()["renditions"], parsed=e.stats()["parsed"], frames=e.stats()["frames"])
    say("== decode_multi4")
    try:
        fresh().decode_multi4(stream(P04), [0, {"orient": 6}], 1)
        result(error=None)
    except RuntimeError as ex:
        result(error=str(ex))


def case_c():
    """Streams with a display orientation SEI in front of the first slice and no orient option: the hand-over of
    the streams without it.  A malformed SEI leaves the stream decodable."""
    for label, sei in (("plain", False), ("sei", True)):
        e = fresh()
        say(f"== {label}")
        ss = []
        for i, codec, k in ((P11, 265, 1), (A11, 264, 3), (P04, 265, 2)):
            s = stream(i)
            ss.append(O.insert_sei(s, codec, 1, 0, k) if sei else s)
        out = e.transcode_multi(ss, [[0, 1]] * 3)
        result(status=e.last_status, sof=[[sof_size(j) for j in item] for item in out],
               orientation=[__import__("h2j").stream_orientation(s) for s in ss])
    e = fresh()
    say("== malformed")
    ss = []
    for i, codec in ((P11, 265), (A11, 264)):
        bad = O.sei_message(47, O.orientation_payload(codec, rotation=0x4000), size=200)
        ss.append(O.insert_nal(stream(i), codec, O.sei_nal(codec, [bad], trailing=False)))
    out = e.transcode_multi(ss, [[{"orient": "auto"}]] * 2)
    result(status=e.last_status, sof=[[sof_size(j) for j in item] for item in out])


# case d: real oriented plans (only a stand-in with the stage shows them; the one without fails these renditions alone).
# Orientations 3, 6 and 7, the last two transposing, on an 8-bit HEVC, a 10-bit HEVC and an H.264 picture
ITEMS_D = [
    # two renditions with one orientation share one oriented source; an oriented window at another orientation
    (P12, [{"orient": 6}, {"orient": 6, "scale": 1}, {"orient": 3, "crop": (2, 2, 60, 30)}, 0]),
    # two K3s levels on an oriented source: a pyramid; a rendition that is oriented, sharpened and raw: K3o, K3u, K3c
    (P04, [{"orient": 7, "scale": 1}, {"orient": 7, "scale": 2}, {"orient": 3, "scale": 1, "sharpen": 16, "format": "rgb"}]),
    (A11, [{"orient": 3}, 1, {"orient": 6, "crop": (16, 16, 32, 32), "scale": 1}]),
]


def case_d():
    import numpy as np
    e = fresh()
    say("== oriented plans")
    out = e.transcode_multi([stream(i) for i, _ in ITEMS_D], [r for _, r in ITEMS_D])
    result(status=e.last_status, sof=[[["px"] + list(j.shape) if isinstance(j, np.ndarray) else sof_size(j) for j in item] for item in out],
           errors=[e.frame_error(o) for o in range(sum(len(r) for _, r in ITEMS_D))],
           renditions=e.stats()["renditions"], parsed=e.stats()["parsed"], frames=e.stats()["frames"])


CASES = {"a": case_a, "b": case_b, "c": case_c, "d": case_d}
ENV = {}

if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "h264-h265-to-jpeg_amd"))
    import h2j
    h2j.load_library()
    CASES[sys.argv[1]]()
