"""HEVC residual parsing around sparse sub-blocks (DESIGN.md §6 "per-bin / per-sub-block cost").

HevcParser::residual() treats the common shapes of a coefficient sub-block on their own paths (one
coefficient as straight-line code, signs of up to two coefficients as single bypass steps, the
coded_sub_block_flag map as one 64-bit word, ...).  The job records must stay bit-identical: the
`parse_bench -r 1 -d` digests below were taken with the parser as it was before that work (df754b6)
for every set tests/test_parse_threads.py does not pin already, and `parse_bench -b` (the counting
build) must show every added path taken by the small vectors."""
import glob
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "h264-h265-to-jpeg_amd", "csrc", "host")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _build(tmp, name, defs):
    exe = str(tmp / name)
    srcs = [os.path.join(ROOT, "tools", "parse_bench", "parse_bench.cpp")] + [
        os.path.join(HOST, f) for f in ("bitstream.cpp", "cabac_tables.cpp", "hevc_parser.cpp", "h264_parser.cpp")]
    subprocess.check_call(["g++", "-O1", "-std=c++11", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", HOST]
                          + defs + srcs + ["-o", exe])
    return exe


@pytest.fixture(scope="module")
def parse_bench(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("pbs"), "parse_bench", [])


@pytest.fixture(scope="module")
def parse_bench_count(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("pbc"), "parse_bench_count", ["-DH2J_CABAC_COUNT"])


def _streams(name):
    return sorted(glob.glob(os.path.join(GOLDEN, name, "*.h26?")))


# (number of streams, digest) at df754b6; hevc_sparse was minted for this file (see below) and
# pinned with the same parent build
PINNED = {
    "bench_aim": (64, "1a63a005aa67e41f"),
    "hevc": (39, "a0fc7d5f3f587832"),
    "bench_nosdh": (2, "44077eafee034c2e"),
    "f3": (7, "965922802c3ecc89"),
    "mixed": (10, "3d711b67e21c23d0"),
    "h264": (45, "4d1ce81093e2f22d"),
    "bench264_heavy": (16, "3a477809e6f37e3f"),
    "h264tall": (None, "4bb443ac1fe10088"),
    "h264wide": (None, "a31670881ec1b894"),
    "entropy": (None, "111fd5515ec7d6d5"),
    "hevc_sparse": (1, "b60c8884e4f0849a"),
}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_parse_records_pinned(parse_bench, name):
    count, digest = PINNED[name]
    paths = _streams(name)
    assert paths and (count is None or len(paths) == count)
    out = subprocess.check_output([parse_bench] + paths + ["-r", "1", "-d"], text=True)
    assert out.split()[-1] == digest


def _breakdown(exe, paths):
    out = subprocess.check_output([exe] + paths + ["-b"], text=True)
    print(out)
    rows = {}
    for line in out.splitlines():
        m = re.match(r"^(\w+)\s+(\d+)\s+(\d+)$", line)
        if m:
            rows[m.group(1)] = int(m.group(3))
    assert re.search(r"^perf: ", out, re.M)  # counters, or the note that the kernel allows none
    return rows, out


def test_breakdown_reproduces_the_bench_aim_counts(parse_bench_count):
    """The counts this work started from: totals over the 64 streams of the headline set."""
    rows, out = _breakdown(parse_bench_count, _streams("bench_aim"))
    assert "digest 1a63a005aa67e41f" in out
    want = {
        "context_bins": 110657447, "bypass_bins": 15854468,
        "tbs_with_residual": 1824411, "sub_blocks_visited": 8864150, "coded_sub_block_flag_bins": 6334344,
        "coded_sub_blocks": 5315647, "sig_coeff_flag_bins_pos_gt0": 67887944, "sig_coeff_flag_bins_pos0": 5177665,
        "greater1_bins": 10618150, "greater2_bins": 1176525, "last_sig_coeff_prefix_bins": 12705010,
        "coefficients": 10858758, "coded_sub_blocks_1_coef": 2854783, "coded_sub_blocks_2_coefs": 1215754,
        "coded_sub_blocks_3_coefs": 563400, "coded_sub_blocks_4_7_coefs": 573939,
        "coded_sub_blocks_8plus_coefs": 107771, "coefs_with_abs_level_remaining": 708845,
        "sub_blocks_with_abs_level_remaining": 241279, "sign_batch_sub_blocks": 1694326,
        "sign_single_sub_blocks": 3621321,
    }
    assert {k: rows.get(k) for k in want} == want
    # every one-coefficient sub-block takes the straight-line path
    assert rows["path_one_coef"] == rows["coded_sub_blocks_1_coef"]


def test_small_vectors_take_every_new_path(parse_bench_count):
    """tests/golden/hevc (72x40 up to 1280x720) reaches each path; the one-coefficient path inside a
    cu_transquant_bypass CU needs a nearly flat picture (a lossless CU with a single non-zero
    difference in a sub-block), which none of them is: tests/golden/hevc_sparse supplies it."""
    rows, _ = _breakdown(parse_bench_count, _streams("hevc"))
    for k in ("path_one_coef", "path_one_coef_escape", "path_one_coef_escape_persistent_rice",
              "path_one_coef_transform_skip", "path_one_coef_escape_transform_skip", "path_dc_only_last_sub_block",
              "path_dc_only_tb", "path_sign_pair_single_steps"):
        assert rows[k] > 0, k
    assert rows["path_one_coef"] == rows["coded_sub_blocks_1_coef"]
    # persistent_rice_adaptation: the escape of a lone coefficient reads and updates StatCoeff
    for pat in ("p29_*", "p30_*"):
        r, _ = _breakdown(parse_bench_count, glob.glob(os.path.join(GOLDEN, "hevc", pat + ".h265")))
        assert r["path_one_coef"] > 0 and r["path_one_coef_transform_skip"] > 0, pat
    r30, _ = _breakdown(parse_bench_count, glob.glob(os.path.join(GOLDEN, "hevc", "p30_*.h265")))
    assert r30["path_one_coef_escape_persistent_rice"] > 0
    # transform skip and transquant bypass, p03 (PCM + bypass + slices) and the sparse picture
    r03, _ = _breakdown(parse_bench_count, glob.glob(os.path.join(GOLDEN, "hevc", "p03_*.h265")))
    assert r03["path_one_coef_escape"] > 0 and r03["path_one_coef_transform_skip"] > 0
    sp, _ = _breakdown(parse_bench_count, _streams("hevc_sparse"))
    assert sp["path_one_coef_transquant_bypass"] > 0 and sp["path_one_coef_escape_transquant_bypass"] > 0


def test_breakdown_needs_the_counting_build(parse_bench):
    """The counters are compiled out of the product build: -b says so there."""
    p = subprocess.run([parse_bench] + _streams("hevc_sparse") + ["-b"], capture_output=True, text=True)
    assert p.returncode == 2 and "H2J_CABAC_COUNT" in p.stderr
