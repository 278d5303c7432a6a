"""CPU: a census of K0's arithmetic (HEVC dequantisation and inverse transforms) over every committed stream, by the
numpy restatement of H.265 8.6.2-8.6.4 in tests/k0_ref.py on the host parser's records (tools/parse_bench/tu_dump).

The census counts the places where the arithmetic has to clip: dequantised values outside int16, first-stage
(column) outputs outside int16, second-stage (row) outputs outside int16, and int16 wraps of transform-skip /
RDPCM residuals.  Every stream older than tests/golden/k0levels/ has none of them, so clipping the second stage
 changes no earlier output.  The k0levels vectors (tools/make_streams.py k0levels, hevcgen
--inject) are there to reach them: tier 1 large but in range, tier 2 past every clip; their conditions are asserted
here from a census recomputed on the spot, which also has to equal the one in their manifest.

Unreachable, with the reason: the cell "4x4 luma, DCT" needs an inter-predicted 4x4 luma block (8.6.4.2 takes the DST
for intra 4x4 luma) and this project decodes intra pictures only; the 4x4 DCT runs on the 4x4 chroma blocks.  A
second-stage output outside int16 needs max column L1 norm * 32767 >> (20 - bitDepth) > 32767 (row_bound below):
never at 8 bits, nor for 4x4 blocks up to 12 bits (DCT 247, DST 242: 31616 and 30976 at 12 bits)."""
import glob
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import k0_ref as K
from conftest import GOLDEN

K0DIR = os.path.join(GOLDEN, "k0levels")
REACHED = [c for c in K.CELLS if c != "luma4dct"]  # (see the module docstring)
SIZE = {"luma4dst": 2, "luma4dct": 2, "luma8": 3, "luma16": 4, "luma32": 5, "chroma4": 2, "chroma8": 3, "chroma16": 4}


@pytest.fixture(scope="module")
def dumper(tmp_path_factory):
    return K.build_dumper(str(tmp_path_factory.mktemp("k0") / "tu_dump"))


def row_bound(cell, bd):
    """the largest second-stage output an int16 first stage allows: max L1 column norm * 32767, shifted"""
    n = 1 << SIZE[cell]
    return (K.l1_max(n, cell == "luma4dst") * 32767 + (1 << (19 - bd))) >> (20 - bd)


def test_transform_matrices():
    """the 32-point matrix against the cosines it approximates, and the bounds the vectors are built around"""
    j, i = np.mgrid[0:32, 0:32]
    exact = 64 * np.sqrt(2) * np.cos((2 * i + 1) * j * np.pi / 64)
    exact[0] = 64
    assert np.abs(K.DCT32 - exact).max() < 2  # (the standard's entries are tuned by up to 1.x from the rounded cosines)
    assert np.array_equal(K.matrix(4), [[64, 64, 64, 64], [83, 36, -36, -83], [64, -64, -64, 64], [36, -83, 83, -36]])
    assert (K.l1_max(4), K.l1_max(4, True)) == (247, 242)
    print("second-stage bound by cell and bit depth:",
          {f"{c}@{bd}": row_bound(c, bd) for c in REACHED for bd in (8, 9, 10, 12)})
    for c in REACHED:
        assert row_bound(c, 8) <= 32767 and row_bound(c, 9) <= 32767  # 8- and 9-bit pictures never leave int16
    assert [c for c in REACHED if row_bound(c, 10) > 32767] == ["luma32"]
    assert [c for c in REACHED if row_bound(c, 12) > 32767] == ["luma8", "luma16", "luma32", "chroma8", "chroma16"]


def _earlier_streams():
    with open(os.path.join(GOLDEN, "parse_digests.json")) as f:
        refused = {k for k, v in json.load(f).items() if v == "error"}
    paths = glob.glob(os.path.join(GOLDEN, "**", "*.h265"), recursive=True) + glob.glob(
        os.path.join(GOLDEN, "**", "*.hevc"), recursive=True)
    rel = sorted(os.path.relpath(p, GOLDEN).replace(os.sep, "/") for p in paths)
    return [r for r in rel if r not in refused and not r.startswith("k0levels/") and not r.startswith("malformed/")]


def test_earlier_streams_never_reach_a_clip(dumper, tmp_path):
    """Zero events of every kind on all HEVC streams that were here before the k0levels vectors; prints the largest
    |level|, dequantised value, first- and second-stage output per cell (the parity vectors tests/golden/hevc apart)."""
    rels = _earlier_streams()
    assert len(rels) >= 170
    pairs = [(os.path.join(GOLDEN, r), str(tmp_path / f"{i}.bin")) for i, r in enumerate(rels)]
    K.dump(dumper, pairs)
    with ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as pool:  # (numpy releases the GIL in the large operations)
        got = list(pool.map(lambda pr: K.census(pr[1]), pairs))
    events, maxima = [], {"hevc/": {}, "all": {}}
    for r, cen in zip(rels, got):
        for cell, rec in cen.items():
            if any(rec[k] for k in K.EVENTS):
                events.append((r, cell, {k: rec[k] for k in K.EVENTS if rec[k]}))
            for scope in ("hevc/", "all"):
                if scope == "all" or r.startswith(scope):
                    m = maxima[scope].setdefault(cell, dict.fromkeys(K.MAXIMA, 0))
                    for k in K.MAXIMA:
                        m[k] = max(m[k], rec[k])
    for scope in maxima:
        for cell in K.CELLS:
            if cell in maxima[scope]:
                print(f"{scope:6s}{cell:9s}", maxima[scope][cell])
    assert not events, events[:8]
    assert set(maxima["all"]) >= set(REACHED)


def _vectors():
    with open(os.path.join(K0DIR, "manifest.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def vectors(dumper, tmp_path_factory):
    """manifest entries with "path" (the tu_dump file), "tb" (one dict per residual block: cell, size, ncoef,
    first coefficient position, flags and the events / maxima of k0_ref.blocks) and "head", "sl" """
    d = tmp_path_factory.mktemp("k0v")
    man = _vectors()
    K.dump(dumper, [(os.path.join(K0DIR, v["file"]), str(d / (v["file"] + ".bin"))) for v in man])
    for v in man:
        v["path"] = str(d / (v["file"] + ".bin"))
        head, tus, coefs, sl = K.load(v["path"])
        v["head"], v["sl"], v["tb"] = head, sl, []
        for log2n in (2, 3, 4, 5):
            b = K.blocks(head, tus, coefs, sl, log2n)
            names = K.cell_names(b, log2n)
            for k, i in enumerate(b["idx"]):
                rec = {"cell": str(names[k]), "log2n": log2n, "ncoef": int(tus[i]["ncoef"]),
                       "pos0": int(coefs[tus[i]["coef"]] >> 16), "tskip": bool(b["tskip"][k]), "bypass": bool(b["bypass"][k])}
                rec.update({e: int(b[e][k]) for e in K.EVENTS + K.MAXIMA})
                v["tb"].append(rec)
    return man


def test_manifest_lists_the_vectors_and_their_census(vectors):
    files = sorted(os.path.basename(p) for p in glob.glob(os.path.join(K0DIR, "*.h265")))
    assert files == sorted(v["file"] for v in vectors)
    for v in vectors:
        assert K.census(v["path"]) == v["census"], v["file"]
        assert (v["head"]["width"], v["head"]["height"], v["head"]["bit_depth"]) == (v["w"], v["h"], v["bit_depth"])
        assert 64 <= v["w"] <= 128 and 64 <= v["h"] <= 128 and v["head"]["log2ctb"] in (5, 6)


def _tbs(vectors, tier, bd, cell):
    return [t for v in vectors if v["tier"] == tier and v["bit_depth"] == bd for t in v["tb"] if t["cell"] == cell]


def _no_event(t):
    return not any(t[e] for e in K.EVENTS)


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_tier1_is_large_and_in_range(vectors, bd):
    """Tier 1: no event anywhere; in every cell a first-stage output of magnitude >= 2^14 that no clip touched, also
    from a single coefficient in a row j >= 1 (90 * 32767 >> 7 = 23039, 83 * 32767 >> 7 = 21247 at N = 4 are the most
    one can give); the four single-corner blocks and a full block per size."""
    for v in vectors:
        if v["tier"] == 1:
            assert all(_no_event(t) for t in v["tb"]), v["file"]
    for cell in REACHED:
        n = 1 << SIZE[cell]
        tbs = [t for t in _tbs(vectors, 1, bd, cell) if not t["tskip"] and not t["bypass"]]
        assert max(t["max_col"] for t in tbs) >= 1 << 14, cell
        single = [t for t in tbs if t["ncoef"] == 1]
        assert max(t["max_col"] for t in single if t["pos0"] >= n) >= 1 << 14, cell
        for corner in (0, n - 1, n * (n - 1), n * n - 1):
            assert any(t["pos0"] == corner and t["max_deq"] >= 1 << 14 for t in single), (cell, corner)
        assert any(t["ncoef"] == n * n for t in tbs), cell


def test_tier1_scaling_lists_and_transform_skip(vectors):
    sl = [v for v in vectors if v["tier"] == 1 and v["head"]["scaling_list"]]
    assert sl and all(v["sl"].min() < 16 < v["sl"].max() for v in sl)
    for v in sl:  # every cell large through its own list
        assert {t["cell"] for t in v["tb"] if t["max_col"] >= 1 << 14} >= set(REACHED), v["file"]
    # transform skip: 4x4 blocks with large levels at every bit depth; at 12 bits up to 32x32, where the shift
    # 15 - bitDepth - log2n is 0 (8x8), -1 and -2: the largest residual uses the int16 range and none wraps
    for bd in (8, 10, 12):
        ts4 = [t for v in vectors if v["tier"] == 1 and v["bit_depth"] == bd for t in v["tb"] if t["tskip"] and t["log2n"] == 2]
        assert max(t["max_deq"] for t in ts4) >= 1 << 14, bd
    big = [t for v in vectors if v["tier"] == 1 and v["bit_depth"] == 12 for t in v["tb"] if t["tskip"] and t["log2n"] > 2]
    for log2n in (3, 4, 5):
        assert max(t["max_deq"] << (log2n - 3) for t in big if t["log2n"] == log2n) >= 1 << 14, log2n
    assert all(t["wrap"] == 0 for t in big)


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_tier2_passes_every_clip(vectors, bd):
    """Tier 2, per cell: blocks with a dequantisation clip of each sign, with a first-stage clip of each sign, and a
    second-stage output outside int16 of each sign exactly where row_bound says one exists; every stream also keeps
    blocks without any event (the batched kernel's group-wide bounds mix both kinds)."""
    for cell in REACHED:
        tbs = _tbs(vectors, 2, bd, cell)
        for e in ("deq_pos", "deq_neg", "col_pos", "col_neg"):
            assert any(t[e] for t in tbs), (cell, e)
        reachable = row_bound(cell, bd) > 32767
        assert any(t["row_pos"] for t in tbs) == reachable and any(t["row_neg"] for t in tbs) == reachable, cell
        if reachable:
            # the bound is met, not only int16 passed (-32768 in the first stage gives a little more than 32767)
            assert max(t["max_row"] for t in tbs) >= row_bound(cell, bd), cell
        assert any(abs(t["max_level"]) == 32768 for t in tbs) and any(t["ncoef"] == 1 << (2 * SIZE[cell]) for t in tbs), cell
    for v in vectors:
        if v["tier"] == 2 and v["bit_depth"] == bd:
            plain = [t for t in v["tb"] if _no_event(t) and not t["tskip"] and not t["bypass"]]
            assert {t["cell"] for t in plain} >= set(REACHED), v["file"]
