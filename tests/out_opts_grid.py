"""The output-options rule as data: the calls of golden/out_opts/grid.txt and how a library answers them.

A grid line is `<call> -> <answer>`.  The call names an entry point and its arguments as plain integers, the option
struct as its int32 words in memory order, so that tests/out_opts_host/out_opts_host.cpp reads the same lines:
    fit  W H fit_w fit_h flags             h2j_fit_size
    win6 W H sei <16 words>                h2j_crop_window6 (h2j_out_opts6)
    win5 W H sei <16 words>                h2j_crop_window5 (h2j_out_opts5)
    win4 W H sei <16 words>                h2j_crop_window4 (h2j_out_opts4)
    win3 W H 0 <12 words>                  h2j_crop_window  (h2j_out_opts3)
    win2 W H 0 <8 words>                   an h2j_out_opts2 item: no entry point takes one without an engine, so the
    win1 W H 0 <2 words>                   library is asked through h2j_crop_window with the h2j_out_opts3 item that has
                                           the same fields and no window (likewise an h2j_out_opts item); the stand-alone
                                           program widens the item itself
The answer is the return code and, when it is 0, `orient x y w h ow oh` (fit: `ow oh`).

The grid is one factor at a time around a few base option sets (calls()); the recording was made with the library of
the commit before the options moved into a module of their own and is never regenerated from the code under test.
"""
import ctypes

FIELDS = ["scale_log2", "max_dim", "fit_w", "fit_h", "flags", "crop_x", "crop_y", "crop_w", "crop_h", "orient", "qscale",
          "sharpen", "format", "r0", "r1", "r2"]
SIZES = [(2, 2), (64, 64), (416, 240), (1920, 1080), (3840, 2160), (65536, 2)]
BASES = [{}, {"scale_log2": 1}, {"fit_w": 100}, {"crop_x": 36, "crop_y": 10, "crop_w": 300, "crop_h": 200},
         {"fit_w": 64, "fit_h": 64, "flags": 2}, {"orient": 6, "scale_log2": 1}]
BOXES = [0, 2, 100, 65535, 65536]
# the fit boxes, one side at a time, and two with both sides
BOX_PAIRS = [(b, 0) for b in BOXES] + [(0, b) for b in BOXES[1:]] + [(100, 60), (65535, 65535)]


def words6(**kw):
    assert set(kw) <= set(FIELDS), kw
    return [kw.get(f, 0) for f in FIELDS]


def variations(W, H):
    """One factor at a time: the fields a variation sets, over whatever the base holds."""
    for orient in range(-1, 10):
        for sei in (0, 6):
            yield sei, {"orient": orient}
    for scale in range(-1, 5):
        for max_dim in (0, 100):
            yield 0, {"scale_log2": scale, "max_dim": max_dim}
    for fw, fh in BOX_PAIRS:
        for flags in range(4):
            yield 0, {"fit_w": fw, "fit_h": fh, "flags": flags}
    # windows: none, even, odd, touching the edges, the whole picture, one sample (pair) outside
    for crop in ((0, 0, 0, 0), (36, 10, 300, 200), (3, 0, 0, 0), (0, 0, 33, 32), (W - 64, H - 32, 64, 32), (0, 0, W, H),
                 (W - 62, 0, 64, 32), (W - 63, 0, 64, 32), (0, H - 30, 64, 32), (0, H, 0, 0), (-2, 0, 0, 0)):
        yield 0, dict(zip(("crop_x", "crop_y", "crop_w", "crop_h"), crop))
    for q in (0, 1, 2, 31, 32):
        yield 0, {"qscale": q}
    for a in (0, 64, 65, -1):
        yield 0, {"sharpen": a}
    for f in range(-1, 4):
        yield 0, {"format": f}
    yield 0, {"format": 1, "qscale": 5}
    for r in ("r0", "r1", "r2"):
        yield 0, {r: 1}


def older_types():
    """Items of each older option type, with a non-zero word in each reserved position among them: (call, words)."""
    W, H = 416, 240
    t1 = [[0, 0], [1, 0], [0, 100], [4, 0], [1, 200]]
    t2 = [s + [0, 0, 0] for s in t1] + [[0, 0, 100, 0, 0], [0, 0, 100, 60, 1], [0, 0, 0, 0, 1], [1, 0, 100, 0, 0], [0, 0, 64, 64, 2]]
    t3 = [s + [0, 0, 0, 0] for s in t2] + [[0, 0, 0, 0, 0, 36, 10, 300, 200], [1, 0, 0, 0, 0, 36, 10, 300, 200],
                                           [0, 0, 64, 64, 2, 100, 0, 0, 0], [0, 0, 0, 0, 0, 3, 0, 0, 0], [0, 0, 0, 0, 0, 400, 0, 64, 32]]
    t4 = [s + [o] for s in t3[5:] for o in (0, 6)] + [[0] * 9 + [o] for o in (-1, 1, 3, 8, 9)]
    t5 = [s + [q, a] for s in t4[::3] for q, a in ((0, 0), (5, 16))] + [[0] * 10 + [q, a] for q, a in ((1, 0), (31, 64), (32, 0), (0, 65))]
    for name, items, nres, seis in (("win1", t1, 0, (0,)), ("win2", t2, 3, (0,)), ("win3", t3, 3, (0,)), ("win4", t4, 6, (0, 6)),
                                    ("win5", t5, 4, (0, 6))):
        for sei in seis:
            for s in items:
                yield f"{name} {W} {H} {sei}", s + [0] * nres
        for k in range(nres):  # a non-zero word in each reserved position, alone and beside valid fields
            for val in (1, -1):
                for s in (items[0], items[-1], items[len(items) // 2]):
                    r = [0] * nres
                    r[k] = val
                    yield f"{name} {W} {H} 0", s + r


def calls():
    out = []
    for W, H in SIZES:
        for fw, fh in BOX_PAIRS:
            for flags in range(4 if (W, H) == (416, 240) else 2):  # (2 and 3 are no flags of h2j_fit_size: once)
                out.append(f"fit {W} {H} {fw} {fh} {flags}")
    for W, H in SIZES + [(3, 2), (2, 65538), (0, 0)]:
        for base in BASES:
            for sei in (0, 6):
                out.append(f"win6 {W} {H} {sei} " + " ".join(map(str, words6(**base))))
    for sei in (-1, 1, 8, 9):
        out.append(f"win6 416 240 {sei} " + " ".join(map(str, words6(orient=-1))))
    for base in BASES[::2]:  # plain, a fit, a cover: the others meet every factor in the sweep of sizes above
        for sei, var in variations(416, 240):
            out.append(f"win6 416 240 {sei} " + " ".join(map(str, words6(**dict(base, **var)))))
    for call, words in older_types():
        out.append(call + " " + " ".join(map(str, words)))
    seen, uniq = set(), []
    for c in out:
        if c not in seen:
            seen.add(c)
            uniq.append(c)
    return uniq


def answer(lib, call):
    """What the loaded libH265ToJpeg.so answers to a call."""
    import h2j
    name, *args = call.split()
    a = [int(x) for x in args]
    ow, oh, ro = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    if name == "fit":
        rc = lib.h2j_fit_size(a[0], a[1], a[2], a[3], a[4], ctypes.byref(ow), ctypes.byref(oh))
        return f"{rc} {ow.value} {oh.value}" if rc == 0 else str(rc)
    W, H, sei, words = a[0], a[1], a[2], a[3:]
    win = (ctypes.c_int32 * 4)()
    if name in ("win1", "win2"):  # the h2j_out_opts3 item with the same fields and no window
        words = words[:2] + [0] * 10 if name == "win1" else words[:5] + [0] * 4 + words[5:8]
        name = "win3"
    buf = (ctypes.c_int32 * len(words))(*words)
    if name == "win3":
        o = h2j.OutOpts3.from_buffer_copy(buf)
        rc = lib.h2j_crop_window(W, H, ctypes.byref(o), win, ctypes.byref(ow), ctypes.byref(oh))
    else:
        fn, typ = {"win4": ("h2j_crop_window4", h2j.OutOpts4), "win5": ("h2j_crop_window5", h2j.OutOpts5),
                   "win6": ("h2j_crop_window6", h2j.OutOpts6)}[name]
        o = typ.from_buffer_copy(buf)
        rc = getattr(lib, fn)(W, H, ctypes.byref(o), sei, win, ctypes.byref(ow), ctypes.byref(oh), ctypes.byref(ro))
    return f"{rc} {ro.value} {win[0]} {win[1]} {win[2]} {win[3]} {ow.value} {oh.value}" if rc == 0 else str(rc)


def grid(lib):
    return "".join(f"{c} -> {answer(lib, c)}\n" for c in calls())


if __name__ == "__main__":  # with H2J_LIB_DIR naming a directory with libH265ToJpeg.so beside a stand-in kernel library
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "h264-h265-to-jpeg_amd"))
    import h2j
    sys.stdout.write(grid(h2j.load_library()))
