"""GPU parity on the sparse lossless picture of tests/golden/hevc_sparse.

sp01 is a 96x64 8-bit picture, flat (Y 120, Cb / Cr 128) except for one sample in thirty moved by
-6..6, coded by tools/hevcgen at QP 30, seed 6, `--bypass 1 --tskip 1 --ctb 16`: its
cu_transquant_bypass CUs hold sub-blocks with a single non-zero difference, several of them with
an escape level, which no other vector has (tests/test_parse_sparse.py counts them).  The oracle
equalled the generator's pre-loop-filter reconstruction when it was minted."""
import glob
import os

import numpy as np
import pytest

import oracle_py as O
from conftest import golden, read

pytestmark = pytest.mark.gpu


def test_sparse_bypass_picture_planes_and_jpeg(engine):
    paths = sorted(glob.glob(os.path.join(golden("hevc_sparse"), "*.h265")))
    assert len(paths) == 1
    s = read(paths[0])
    for stage, skip in ((1, True), (0, False)):
        gy, gu, gv, bd = engine.decode(s, stage=stage)
        oy, ou, ov, obd = O.decode(s, 265, skip_loop_filter=skip)
        assert bd == obd == 8
        for g, o, name in ((gy, oy, "Y"), (gu, ou, "U"), (gv, ov, "V")):
            diff = np.argwhere(g != o)
            assert diff.size == 0, f"stage {stage} {name}: {len(diff)} mismatches, first {diff[:4].tolist()}"
    assert engine.transcode([s])[0] == O.transcode(s)
