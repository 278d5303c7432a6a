"""GPU: K0's dequantisation and inverse transforms at levels up to the int16 range (tests/golden/k0levels, what each
vector reaches is asserted on the CPU by tests/test_k0_levels.py): large values inside every clip (tier a*), and past the
dequantisation clip, the clip between the two transform stages and the int16 range after the second one (tier b*),
where K0 clips as the oracle and FFmpeg's template do.  Integer work: bit-exact."""
import glob
import os

import numpy as np
import pytest

import oracle_py as O
from conftest import golden, read

pytestmark = pytest.mark.gpu

VECTORS = sorted(glob.glob(os.path.join(golden("k0levels"), "*.h265")))


def test_vectors_present():
    assert len(VECTORS) == 9


@pytest.mark.parametrize("path", VECTORS, ids=[os.path.basename(p) for p in VECTORS])
def test_planes_and_jpeg_equal_the_oracle(engine, path):
    s = read(path)
    for stage, skip in ((1, True), (0, False)):
        gy, gu, gv, bd = engine.decode(s, stage=stage)
        oy, ou, ov, obd = O.decode(s, 265, skip_loop_filter=skip)
        assert bd == obd
        for g, o, name in ((gy, oy, "Y"), (gu, ou, "U"), (gv, ov, "V")):
            diff = np.argwhere(g != o)
            assert diff.size == 0, f"stage {stage} {name}: {len(diff)} mismatches, first {diff[:4].tolist()}"
    assert engine.transcode([s])[0] == O.transcode(s)


def test_one_batch_with_ordinary_pictures(engine):
    """the vectors interleaved with ordinary pictures of other sizes and bit depths in one batch (K1's picture pool
    and the merged launch do not depend on the content): every JPEG byte-exact"""
    hevc = sorted(glob.glob(os.path.join(golden("hevc"), "*.h265")))
    plain = [p for p in hevc if os.path.basename(p)[:3] in ("p01", "p04", "p27")] + [golden("img01.h265")]
    assert len(plain) == 4
    paths = [p for i, v in enumerate(VECTORS) for p in ([v, plain[i % 4]])]
    streams = [read(p) for p in paths]
    outs = engine.transcode(streams)
    for s, o, p in zip(streams, outs, paths):
        assert o is not None, p
        assert o == O.transcode(s), p
