"""The cases of test_engine_handover.py: what the host engine hands to the GPU library, call by call.

Run as `python handover_cases.py <case>` with H2J_LIB_DIR naming a directory that holds libH265ToJpeg.so
beside the host-memory stand-in for libh2j_hip.so (tests/fake_gpu/fake_gpu.cpp).  Everything goes to
stderr, in order: a `== label` line per call, the stand-in's transcript of the call, and a `result` line
(JSON) with what the call returned -- statuses and the SOF size of every JPEG.  Every call that takes an
Engine gets a fresh one: a reused engine leaves earlier bytes in the alignment gaps of its staging buffer,
and the digests would depend on the call history.

The module is also imported by the test for the tables below (streams, their cropped sizes, options).
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")

# stream -> cropped luma size (None: does not parse)
POOL = [
    ("hevc/p11_64x64_tiny.h265", (64, 64)),                    # smallest HEVC picture
    ("hevc/p12_72x40_odd_crop.h265", (72, 40)),                # crop: no variance fold
    ("hevc/p04_416x240_10bit_ctb32_d2.h265", (416, 240)),      # high bit depth
    ("hevc/p19_480x272_tiles2x2_wpp_nolf.h265", (480, 272)),   # no SAO plane
    ("bench4k/hevc2160_10b_03.h265", (3840, 2160)),            # taller than 1088: two-entry K1 form
    ("h264/a11_64x64_tiny.h264", (64, 64)),                    # smallest H.264 picture
    ("h264/a04_352x288_10bit_high10.h264", (352, 288)),        # high bit depth
    ("h264/a31_336x192_mbaff_cabac_8x8.h264", (336, 192)),     # MBAFF
    ("h264tall/t01_256x1152_tall_10bit.h264", (256, 1152)),    # banded K1, xline
    ("h264tall/t02_192x1408_tall_cavlc.h264", (192, 1408)),
    ("malformed/m_hevc_bitdepth11.h265", None),                # a parse failure in the batch
]
P11, P12, P04, P19, P4K, A11, A04, A31, T01, T02, BAD = range(11)

# case b: per-item (scale, max_dim, fit, stretch) of POOL
OPTS_B = [
    (1, 0, None, False),             # scale 1
    (0, 0, (50, 0), False),          # a fit: K3r
    (0, 200, None, False),           # max_dim: resolves to scale 2
    (0, 0, (100, 60), True),         # a stretch fit
    (0, 0, (1920, 1080), False),     # a fit that resolves to K3s level 1
    (5, 0, None, False),             # invalid
    (3, 0, None, False),
    (0, 0, (0, 100), False),         # the height binds
    (0, 0, None, False),
    (1, 400, None, False),           # max_dim from scale 1 up: 2
    (1, 0, None, False),             # the malformed item
]

# case c: per-item rendition lists of POOL (h2j.rendition_spec)
RENDS_C = [
    [0, 1, 2, 3],                                                  # a pyramid plus the unscaled view
    [1, 1],                                                        # a duplicate
    [(50, 0), 1],
    [1, 7, 0],                                                     # one invalid rendition among valid ones
    [9, {"scale": 1, "fit": (10, 10)}],                            # all invalid: the item is not parsed
    [0],
    [2, 3],                                                        # a pyramid without the unscaled view
    [(100, 60), {"fit": (100, 60), "stretch": True}, 0],
    [1],
    [0, 0],
    [0, 1],                                                        # the malformed item
]

CHUNKED_E = [P11, P12, A11, P04, A04]  # with H2J_CHUNK=2: three chunks, both slots, the `after` wait

# case f: the C entry points of the request queue (decoder.cpp), (function, stream, arguments)
MEM_F = [
    ("mem", P11, ()),
    ("mem_scaled", P04, (1, 0)),
    ("mem_fit", P19, (100, 0, 0)),
    ("mem_multi", A04, [0, 1, 7, (50, 0)]),
    ("mem", BAD, ()),
]


def stream(i):
    with open(os.path.join(GOLDEN, POOL[i][0]), "rb") as f:
        return f.read()


def say(line):
    sys.stderr.write(line + "\n")
    sys.stderr.flush()


def sof_size(jpeg):
    """(width, height) of the JPEG's baseline SOF0 segment; None for no JPEG."""
    if jpeg is None:
        return None
    assert jpeg[:2] == b"\xff\xd8", "not a JPEG"
    p = 2
    while p + 4 <= len(jpeg):
        assert jpeg[p] == 0xFF, "lost JPEG marker sync"
        marker, seglen = jpeg[p + 1], int.from_bytes(jpeg[p + 2:p + 4], "big")
        if marker == 0xC0:
            return [int.from_bytes(jpeg[p + 7:p + 9], "big"), int.from_bytes(jpeg[p + 5:p + 7], "big")]
        if marker == 0xDA:
            break
        p += 2 + seglen
    raise AssertionError("no SOF0 segment")


def result(**kw):
    say("result " + json.dumps(kw, sort_keys=True))


def fresh():
    import h2j
    return h2j.Engine(0, 2)


def case_a():
    e = fresh()
    say("== transcode pool")
    out = e.transcode([stream(i) for i in range(len(POOL))])
    result(status=e.last_status, sof=[sof_size(j) for j in out])


def case_b():
    e = fresh()
    say("== transcode pool, per-item options")
    out = e.transcode([stream(i) for i in range(len(POOL))], scale=[o[0] for o in OPTS_B],
                      max_dim=[o[1] for o in OPTS_B], fit=[o[2] for o in OPTS_B], stretch=[o[3] for o in OPTS_B])
    result(status=e.last_status, sof=[sof_size(j) for j in out],
           errors=[e.frame_error(i) for i in range(len(POOL))])


def case_c():
    e = fresh()
    say("== transcode_multi pool")
    out = e.transcode_multi([stream(i) for i in range(len(POOL))], RENDS_C)
    result(status=e.last_status, sof=[[sof_size(j) for j in item] for item in out],
           parsed=e.stats()["parsed"], renditions=e.stats()["renditions"],
           errors=[e.frame_error(o) for o in range(sum(len(x) for x in RENDS_C))])


def case_d():
    say("== decode stage 1")
    y, u, v, bd = fresh().decode(stream(P12), 1)
    result(shape=list(y.shape), bit_depth=int(bd))
    say("== decode_batch")
    y, u, v, bd = fresh().decode_batch([stream(P11), stream(A11), stream(T01)], 1)
    result(shape=list(y.shape), bit_depth=int(bd))
    say("== jpeg_coeffs")
    r = fresh().jpeg_coeffs(stream(A04))
    result(shape=list(r[1].shape))
    say("== decode_scaled")
    r = fresh().decode_scaled(stream(P04), 2)
    result(shape=list(r[0].shape), scale=int(r[3]))
    say("== decode_resized")
    r = fresh().decode_resized(stream(P19), (100, 0))
    result(shape=list(r[0].shape))
    say("== decode_multi, a pick inside a pyramid")
    y, u, v, size, mode = fresh().decode_multi(stream(P04), [0, 1, 2, (50, 0)], 2)
    result(size=list(size), mode=mode)


def case_e():
    e = fresh()
    say("== transcode, chunks of 2")
    out = e.transcode([stream(i) for i in CHUNKED_E])
    result(status=e.last_status, sof=[sof_size(j) for j in out], chunks=e.stats()["chunks"])


def case_f():
    import h2j
    lib = h2j.load_library()
    u8p = ctypes.POINTER(ctypes.c_uint8)

    def take(p, n):
        jpeg = ctypes.string_at(p, n.value if hasattr(n, "value") else n)
        lib.h2j_free(ctypes.cast(p, ctypes.c_void_p))
        return jpeg

    for name, i, args in MEM_F:
        say("== h2j_h265_to_jpeg_" + name)
        s = stream(i)
        buf = h2j._u8(s)
        if name == "mem_multi":
            _, opts, n = h2j._multi_opts([[h2j.rendition_spec(x) for x in args]])
            jp, ln, st = (u8p * n)(), (ctypes.c_size_t * n)(), (ctypes.c_int * n)()
            rc = lib.h2j_h265_to_jpeg_mem_multi(buf, len(s), n, opts, jp, ln, st)
            result(rc=rc, status=list(st), sof=[sof_size(take(jp[r], ln[r])) if st[r] == 0 else None for r in range(n)])
            continue
        jp, ln = u8p(), ctypes.c_size_t(0)
        if name == "mem":
            lib.h2j_h265_to_jpeg_mem.restype = ctypes.c_int
            lib.h2j_h265_to_jpeg_mem.argtypes = [u8p, ctypes.c_size_t, ctypes.POINTER(u8p), ctypes.POINTER(ctypes.c_size_t)]
            rc = lib.h2j_h265_to_jpeg_mem(buf, len(s), ctypes.byref(jp), ctypes.byref(ln))
        elif name == "mem_scaled":
            rc = lib.h2j_h265_to_jpeg_mem_scaled(buf, len(s), args[0], args[1], ctypes.byref(jp), ctypes.byref(ln))
        else:
            rc = lib.h2j_h265_to_jpeg_mem_fit(buf, len(s), args[0], args[1], args[2], ctypes.byref(jp), ctypes.byref(ln))
        result(rc=rc, sof=sof_size(take(jp, ln)) if rc == 0 else None)


CASES = {"a": case_a, "b": case_b, "c": case_c, "d": case_d, "e": case_e, "f": case_f}
ENV = {"e": {"H2J_CHUNK": "2"}, "f": {"H2J_ENGINES": "1"}}  # what the test sets for a case's child

if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "h264-h265-to-jpeg_amd"))
    import h2j
    h2j.load_library()  # the stand-in's first transcript line comes before any label
    CASES[sys.argv[1]]()
