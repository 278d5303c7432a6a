"""Branch sites of the HEVC slice-data path (DESIGN.md §6 "branch sites").

A `-DH2J_CABAC_COUNT` build gives every data-dependent branch of residual coding, the transform tree, the coding
unit and the coding quadtree a named counter (cabac.h H2J_BRANCH_SITES): executions, times taken, and the misses of
a two-bit predictor simulated per site, so the numbers are the same on every machine.  `parse_bench -B` prints them.
tests/golden/parse_branch_sites.json is the table of the 64 bench_aim streams that DESIGN.md §6 shows."""
import glob
import json
import os
import re
import subprocess

import pytest

from conftest import GOLDEN, PKG, ROOT

HOST = os.path.join(PKG, "csrc", "host")


def _build(tmp, name, defs):
    exe = str(tmp / name)
    srcs = [os.path.join(ROOT, "tools", "parse_bench", "parse_bench.cpp")] + [
        os.path.join(HOST, f) for f in ("bitstream.cpp", "cabac_tables.cpp", "hevc_parser.cpp", "h264_parser.cpp")]
    subprocess.check_call(["g++", "-O1", "-std=c++11", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", HOST]
                          + defs + srcs + ["-o", exe])
    return exe


@pytest.fixture(scope="module")
def parse_bench_count(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("pbb"), "parse_bench_count", ["-DH2J_CABAC_COUNT"])


def _sites(exe, paths):
    out = subprocess.check_output([exe] + paths + ["-B"], text=True)
    rows = {}
    for line in out.splitlines():
        m = re.match(r"^(\w+)\s+(\d+)\s+(\d+)\s+(\d+)\s+\d+$", line)
        if m:
            rows[m.group(1)] = [int(m.group(k)) for k in (2, 3, 4)]
    return rows, out


def test_bench_aim_table_is_the_committed_one(parse_bench_count):
    paths = sorted(glob.glob(os.path.join(GOLDEN, "bench_aim", "*.h265")))
    assert len(paths) == 64
    rows, out = _sites(parse_bench_count, paths)
    print(out)
    assert "digest 1a63a005aa67e41f" in out
    with open(os.path.join(GOLDEN, "parse_branch_sites.json")) as f:
        want = json.load(f)
    assert rows == want
    total = rows.pop("all_sites")
    assert total == [sum(r[k] for r in rows.values()) for k in range(3)]
    for name, (executed, taken, misses) in rows.items():
        assert taken <= executed and misses <= executed, name


def test_no_site_is_dead_on_the_small_vectors(parse_bench_count):
    """The parity vectors (tests/golden/hevc/p*.h265, 72x40 and up) reach every site, and the sites the issue
    names are all there."""
    paths = sorted(glob.glob(os.path.join(GOLDEN, "hevc", "p*.h265")))
    assert paths
    rows, _ = _sites(parse_bench_count, paths)
    for name, (executed, taken, _) in rows.items():
        assert executed > 0, name
        assert taken <= executed, name
    for name in ("csbf_coded_range", "sub_block_uncoded", "infer_dc", "sub_block_empty", "one_coef_split", "one_coef_g1",
                 "one_coef_g2", "g1_second_bin", "g1_loop", "g1_any", "signs_gt2", "escape_loop", "output_loop",
                 "last_x_max", "last_x_bin", "last_y_max", "last_y_bin", "last_x_suffix", "last_y_suffix",
                 "decision_refill", "tt_split", "tt_cbf_cb_coded", "tt_cbf_cr_coded", "cu_prev_intra", "cu_mpm_idx0",
                 "cu_cand_equal", "cq_split"):
        assert name in rows, name


def test_site_table_needs_the_counting_build(tmp_path):
    """The counters are compiled out of the product build: -B says so there, as -b does."""
    exe = _build(tmp_path, "parse_bench", [])
    p = subprocess.run([exe] + glob.glob(os.path.join(GOLDEN, "hevc_sparse", "*.h265")) + ["-B"], capture_output=True,
                       text=True)
    assert p.returncode == 2 and "H2J_CABAC_COUNT" in p.stderr
