"""GPU: HEIF / HEIC input (DESIGN.md "HEIF input").

A single-item file must give the bytes of the Annex-B call.  A grid is handed to the GPU as one tiled canvas picture:
its decoded planes must equal, bit for bit, the oracle's decode of every tile on its own, composed and cropped in numpy
(tests/heif_ref.py), and its JPEG the bytes the oracle's encoder makes of those planes.  Every other expectation is
those planes through the existing reference modules; nothing here is another call into the engine."""
import functools

import numpy as np
import pytest

import crop_ref as C
import heif_mux as M
import heif_ref as HR
import oracle_py as O
import orient_ref as OR
import resize_ref as RS
import rgb_ref as RGB
import scale_ref as S
from conftest import golden, read

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def grid_file(name, cols, rows, W, H, irot=None):
    tr = [("irot", irot)] if irot is not None else []
    return M.mux(list(HR.tiles(name))[:cols * rows], grid=(rows, cols, W, H), transforms=tr)


@functools.lru_cache(maxsize=None)
def grid_jpeg(case):
    y, u, v, bd = HR.canvas(*case)
    return S.encode(*S.scale_planes(y, u, v, bd, 0))


def case_of(name):
    return next(c for c in HR.CASES if c[0] == name)


# 4. single items: the bytes of the Annex-B calls
def test_single_items_equal_the_annexb_calls(engine):
    names = [("img01.h265", 265), ("img01.h264", 264), ("hevc/p11_64x64_tiny.h265", 265), ("h264/a12_72x40_odd_crop.h264", 264),
             ("hevc/p08_320x180_10bit_q2.h265", 265)]
    streams = [read(golden(n)) for n, _ in names]
    files = [M.mux([s], codec=c, **k) for s, (_, c) in zip(streams, names)
             for k in ({}, dict(iloc_version=2, construction=1, mdat_first=True, thumb=True))]
    want = engine.transcode(streams)
    assert want == [O.transcode(s) for s in streams]
    got = engine.transcode(files)
    assert got == [w for w in want for _ in range(2)], [engine.frame_error(i) for i in range(len(files))]


# 5. grids: planes against the composed oracle decode, JPEG against the oracle's encoder on those planes
@pytest.mark.parametrize("case", HR.CASES, ids=lambda c: f"{c[0]}_{c[1]}x{c[2]}")
def test_grid_planes_and_jpeg_bit_exact(engine, case):
    data = grid_file(*case)
    ey, eu, ev, bd = HR.canvas(*case)
    y, u, v, gbd = engine.decode(data)
    assert gbd == bd
    for g, e, pl in ((y, ey, "Y"), (u, eu, "U"), (v, ev, "V")):
        assert g.shape == e.shape, (pl, g.shape, e.shape)
        diff = np.argwhere(g != e)
        assert diff.size == 0, f"{pl}: {len(diff)} mismatches, first at {diff[:5].tolist()}"
    (jpeg,) = engine.transcode([data])
    assert jpeg == grid_jpeg(case), engine.frame_error(0)


def test_grids_in_one_batch(engine):
    outs = engine.transcode([grid_file(*c) for c in HR.CASES])
    assert outs == [grid_jpeg(c) for c in HR.CASES], [engine.frame_error(i) for i in range(len(outs))]


# 6. set e, irot = 1 muxed in: renditions through the reference modules applied to the canvas
def test_renditions_of_a_grid(engine):
    import h2j
    case = case_of("e")
    data = grid_file(*case, irot=1)
    assert h2j.stream_orientation(data) == 8  # 90 degrees anticlockwise
    specs = [0, 2, {"cover": (128, 128)}, {"fit": (224, 224), "format": "rgb"}, {"orient": "auto"}]
    y, u, v, bd = HR.canvas(*case)
    (outs,) = engine.transcode_multi([data], [specs])
    assert all(st == 0 for st in engine.last_status[0]), engine.last_status
    for spec, got in zip(specs, outs):
        geo = spec if isinstance(spec, int) else {k: val for k, val in spec.items() if k != "format"}
        win, (ow, oh), mode, o = OR.resolve(y.shape[1], y.shape[0], sei=8, **OR.spec_fields(geo))
        wy, wu, wv = C.window_planes(*OR.orient_planes(y, u, v, o), win)
        planes = RS.resize_planes(wy, wu, wv, bd, ow, oh) if mode == C.RESAMPLE else S.scale_planes(wy, wu, wv, bd, mode)
        if isinstance(spec, dict) and spec.get("format"):
            want = RGB.convert(*planes, "rgb")
            assert isinstance(got, np.ndarray) and got.shape == want.shape and np.array_equal(got, want), spec
        else:
            assert got == S.encode(*planes), spec
    # the file's orientation is never applied unasked: rendition 0 is the upright canvas; "auto" turned it
    assert O.jpeg_parse(outs[0])[:2] == (700, 500) and O.jpeg_parse(outs[4])[:2] == (500, 700)


# 7. one batch of a grid, an Annex-B stream, a truncated file and a Main10 grid with two slices per tile
def test_mixed_batch_with_a_truncated_file(engine):
    a, d = case_of("a"), case_of("d")
    img = read(golden("img01.h265"))
    whole = M.mux([read(golden("hevc/p11_64x64_tiny.h265"))])
    outs = engine.transcode([grid_file(*a), img, whole[:len(whole) // 3], grid_file(*d)])
    assert outs[2] is None and engine.last_status[2] < 0
    assert engine.frame_error(2) == "HEIF: truncated or malformed box structure"
    assert outs[0] == grid_jpeg(a) and outs[1] == O.transcode(img) and outs[3] == grid_jpeg(d)
    assert [engine.frame_error(i) for i in (0, 1, 3)] == ["", "", ""]
