"""The finishing cases of test_finish_api.py: what the host engine hands to the GPU library when renditions carry
qscale or sharpen, in the way handover_cases.py does it (same transcript, a fresh Engine per call).  Run as
`python finish_handover_cases.py <case>` with H2J_LIB_DIR naming the stand-in's directory: case a against
tests/fake_gpu/fake_gpu.cpp, a kernel library without the finishing stage; cases b and c against
tests/fake_gpu/fake_gpu_finish.cpp, which has it.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from handover_cases import POOL, P11, P12, P04, A04, A11, BAD, fresh, result, say, sof_size, stream  # noqa: E402

# case a: finishing renditions among plain items, against a kernel library without the stage
ITEMS_A = [
    (P11, [0, 1]),
    (P04, [0, {"sharpen": 16}, {"crop": (36, 10, 300, 200), "scale": 1}, {"qscale": 5, "scale": 1}]),
    (BAD, [0]),
    (A04, [{"qscale": 40}, 1]),
    (P12, [{"sharpen": 8, "scale": 1}]),   # every rendition of the item is finished: the item gets no frame
]

# case b: one fixed chunk.  Views in plan order (frame-major, the plain unscaled view of a frame first):
#   P12 72 x 40:    0 plain | 1 scale 1 sharpen 16 (wide) | 2 qscale 7
#   P04 416 x 240:  3 plain | 4 sharpen 32 (16-bit source) | 5 scale 1 qscale 31 sharpen 8 (wide) | 6 scale 2
#   A11 64 x 64:    7 sharpen 64 (8-bit source, its frame's first view)
ITEMS_B = [
    (P12, [{"scale": 1, "sharpen": 16}, 0, {"qscale": 7}]),
    (P04, [{"sharpen": 32}, {"scale": 1, "qscale": 31, "sharpen": 8}, 0, 2, {"sharpen": 32}]),
    (A11, [{"sharpen": 64}]),
]
QFORCE_B = [0, 0, 7, 0, 0, 31, 0, 0]
# the K3u map by class: wide, 8-bit, 16-bit
FIN_B = ["fin 36 20 sharpen 16 depth 8,8 wide 1 crop 0,0 pitch 48/48,32,32 own 1",
         "fin 208 120 sharpen 8 depth 8,8 wide 1 crop 0,0 pitch 208/208,112,112 own 1",
         "fin 64 64 sharpen 64 depth 8,8 wide 0 crop 0,0 pitch 64/64,32,32 own 1",
         "fin 416 240 sharpen 32 depth 10,10 wide 0 crop 0,0 pitch 416/416,208,208 own 1"]

# case c: the same call through the multi4 call and through multi5 with both options 0
SAME_C = ([P11, P04, A04], [[0], [1, 2, {"crop": (36, 10, 300, 200)}], [{"cover": (64, 64)}, {"orient": 0, "fit": (50, 0)}]],
          [[{"qscale": 0}], [{"sharpen": 0, "scale": 1}, {"qscale": 0, "sharpen": 0, "scale": 2}, {"qscale": 0, "crop": (36, 10, 300, 200)}],
           [{"sharpen": 0, "cover": (64, 64)}, {"qscale": 0, "orient": 0, "fit": (50, 0)}]])


def finished(spec):
    return isinstance(spec, dict) and bool(spec.get("qscale") or spec.get("sharpen"))


def without_finished(specs):
    return [s for s in specs if not finished(s)]


def run(label, items):
    e = fresh()
    say(f"== {label}")
    out = e.transcode_multi([stream(i) for i, _ in items], [r for _, r in items])
    result(status=e.last_status, sof=[[sof_size(j) for j in item] for item in out],
           errors=[e.frame_error(o) for o in range(sum(len(r) for _, r in items))],
           renditions=e.stats()["renditions"], parsed=e.stats()["parsed"], frames=e.stats()["frames"])


def case_a():
    run("with the finishing renditions", ITEMS_A)
    run("without the finishing renditions", [(i, without_finished(r)) for i, r in ITEMS_A if without_finished(r)])
    say("== decode_multi5")
    try:
        fresh().decode_multi5(stream(P04), [0, {"sharpen": 16}], 1)
        result(error=None)
    except RuntimeError as ex:
        result(error=str(ex))


def case_b():
    run("fixed chunk", ITEMS_B)


def case_c():
    idx, plain, zero = SAME_C
    for label, rend in (("plain", plain), ("zero", zero)):
        run(label, list(zip(idx, rend)))


CASES = {"a": case_a, "b": case_b, "c": case_c}

if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "h264-h265-to-jpeg_amd"))
    import h2j
    h2j.load_library()
    CASES[sys.argv[1]]()
