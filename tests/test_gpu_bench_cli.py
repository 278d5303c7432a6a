"""GPU: bench.py's command line on a 4-picture batch -- --steps sets the timed steps, a plain run
prints the headline line only, --full adds what it did before, --dump-outputs writes the last
timed step's JPEGs (status, length, CRC-32, sampled bytes) and they equal the oracle's."""
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import oracle_py as O
from conftest import ROOT, golden, read

pytestmark = pytest.mark.gpu

FRAMES = 4
FULL_ONLY = ("outputs_verified", "outputs_checked", "single_call_ms", "value_light", "host_thread_sweep_fps",
             "cpu_baseline")


def _bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--frames", str(FRAMES)]
                       + list(extra), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    d = tmp_path_factory.mktemp("dump")
    return _bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(d)), d


def test_plain_run_headline_only(plain):
    res, _ = plain
    assert res["steps"] == 3 and res["warmup"] == 1
    assert res["unit"] == "frames/s" and res["higher_is_better"] is True and res["dtype"] == "u8"
    assert res["ms_per_step"] > 0
    # value and ms_per_step describe the same 3 timed steps of FRAMES pictures
    assert res["value"] == pytest.approx(FRAMES / (res["ms_per_step"] / 1e3), rel=1e-6)
    assert not [k for k in FULL_ONLY if k in res]


def test_dump_outputs_equal_the_oracle(plain):
    _, d = plain
    streams = [read(golden(f"bench_aim/hevc1080a_{i:02d}.h265")) for i in range(FRAMES)]
    ref = [O.transcode(s) for s in streams]
    got = {n: np.load(d / f"{n}.npy") for n in ("jpeg_status", "jpeg_lens", "jpeg_crc32", "jpeg_sample_index",
                                                 "jpeg_sample_bytes")}
    assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= 64 * 1000 * 1000
    assert got["jpeg_status"].tolist() == [0] * FRAMES
    assert got["jpeg_lens"].tolist() == [len(j) for j in ref]
    assert got["jpeg_crc32"].tolist() == [zlib.crc32(j) for j in ref]
    assert got["jpeg_sample_index"].tolist() == list(range(FRAMES))  # 4 pictures fit the sample whole
    assert got["jpeg_sample_bytes"].dtype == np.float32
    assert got["jpeg_sample_bytes"].astype(np.uint8).tobytes() == b"".join(ref)


def test_full_run_keeps_the_extra_measurements():
    res = _bench("--steps", "1", "--warmup", "0", "--full", "--no-cpu-baseline")
    assert res["steps"] == 1 and res["outputs_verified"] is True
    assert res["outputs_checked"]["pictures"] == FRAMES
    assert set(res["single_call_ms"]) == {"img01.h265", "workload_stream0"}
    assert res["value_light"] > 0 and res["host_thread_sweep_fps"]
    assert "cpu_baseline" not in res
