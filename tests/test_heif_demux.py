"""The HEIF demuxer (csrc/host/heif.cpp) alone, through the stand-alone program tests/heif_host/heif_host.cpp.

Files come from the independent muxer tests/heif_mux.py: for every variant of the box syntax the demuxed Annex-B bytes
must be the source stream's NAL units and the geometry what was muxed; every rejection gives its message; every
truncation and every single-byte mutation of the `meta` box ends in an error or a result inside the buffer.  The same
corpus runs a second time through a build with -fsanitize=address,undefined (a stand-alone host program)."""
import resource
import struct
import subprocess

import numpy as np
import pytest

import heif_host_build as B
import heif_mux as M
import heif_ref as HR
import orient_ref as OR
from conftest import golden, read

P11 = read(golden("hevc/p11_64x64_tiny.h265"))
A11 = read(golden("h264/a11_64x64_tiny.h264"))
B0 = HR.tiles("b")[0]  # every NAL unit shorter than 256 bytes: length size 1
SET_A = list(HR.tiles("a"))
GRID_A = (2, 2, 120, 100)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return B.build(tmp_path_factory.mktemp("heif_host"))


@pytest.fixture(scope="module")
def host_san(tmp_path_factory):
    return B.build(tmp_path_factory.mktemp("heif_host_san"), "heif_host_san", B.SANITIZE)


def demux(exe, tmp, data, limit_mib=0):
    """the program's answer as a dict; limit_mib: run it with that much address space (not for sanitizer builds)"""
    path = str(tmp / "in.heic")
    with open(path, "wb") as f:
        f.write(data)
    cap = (lambda: resource.setrlimit(resource.RLIMIT_AS, (limit_mib << 20, limit_mib << 20))) if limit_mib else None
    p = subprocess.run([exe, "demux", path], capture_output=True, text=True, preexec_fn=cap)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-2000:])
    r = {"tiles": [], "spans": []}
    for line in p.stdout.splitlines():
        k, _, v = line.partition(" ")
        if k == "tile":
            r["tiles"].append(bytes.fromhex(v))
        elif k == "span":
            r["spans"].append(tuple(int(x) for x in v.split()))
        elif k == "codec":
            w = line.split()
            r.update({w[i]: int(w[i + 1]) for i in range(0, len(w), 2)})
        elif k in ("heif", "status"):
            r[k] = int(v)
        else:
            r[k] = v
    return r


SINGLE = {
    "plain": {},
    "iloc_v1_idat": dict(iloc_version=1, construction=1),
    "iloc_v2_wide": dict(iloc_version=2, offset_size=8, length_size=8),
    "base_offset4": dict(base_offset_size=4),
    "base_offset8_no_offset": dict(base_offset_size=8, offset_size=0),
    "index_size": dict(iloc_version=1, index_size=4),
    "index_size8_v2": dict(iloc_version=2, index_size=8, base_offset_size=4, extents=2),
    "extents3": dict(extents=3),
    "extents4_base8_v1": dict(iloc_version=1, extents=4, base_offset_size=8),
    "infe_v3": dict(infe_version=3),
    "pitm_v1": dict(pitm_version=1),
    "ipma_v1": dict(ipma_version=1),
    "ipma_wide": dict(ipma_wide=True),
    "ipma_v1_wide": dict(ipma_version=1, ipma_wide=True),
    "largesize": dict(largesize=True),
    "mdat_first": dict(mdat_first=True),
    "mdat_first_largesize": dict(mdat_first=True, largesize=True, extents=2),
    "thumb_aux": dict(thumb=True, aux=True),
    "length2": dict(nal_length_size=2),
    "clap_essential": dict(clap=True),
    "brand_mif1": dict(brand=b"mif1"),
    "sei_in_item": dict(sei_in_config=False),
}
GRID = {
    "plain": {},
    "grid32": dict(grid32=True),
    "descriptor_in_mdat": dict(grid_construction=0),
    "tiles_in_idat_v2": dict(iloc_version=2, construction=1, infe_version=3, ipma_version=1, pitm_version=1),
    "thumb_aux_extents": dict(thumb=True, aux=True, extents=2, mdat_first=True),
    "length2_wide": dict(nal_length_size=2, ipma_wide=True, largesize=True),
}


@pytest.mark.parametrize("name", sorted(SINGLE))
def test_single_item_variants(host, tmp_path, name):
    k = SINGLE[name]
    for stream, codec in ((P11, 265), (A11, 264)):
        data = M.mux([stream], codec=codec, **k)
        r = demux(host, tmp_path, data)
        assert r["heif"] == 1 and r["status"] == 0, r["message"]
        assert (r["codec"], r["grid"], r["rows"], r["cols"], r["orient"]) == (codec, 0, 1, 1, 0)
        assert r["tiles"] == [M.expected_annexb(stream, codec, k.get("sei_in_config", True))]
        assert all(o + n <= len(data) for o, n in r["spans"])


def test_single_item_is_the_streams_nal_units(host, tmp_path):
    """for the project's streams (parameter sets, then slices) the rewritten stream is the source's NAL unit list"""
    for stream, codec in ((P11, 265), (A11, 264), (read(golden("img01.h265")), 265)):
        r = demux(host, tmp_path, M.mux([stream], codec=codec))
        assert M.split_nals(r["tiles"][0]) == M.split_nals(stream)


def test_length_size_1(host, tmp_path):
    r = demux(host, tmp_path, M.mux([B0], nal_length_size=1))
    assert r["status"] == 0 and r["tiles"] == [M.expected_annexb(B0)]


@pytest.mark.parametrize("name", sorted(GRID))
def test_grid_variants(host, tmp_path, name):
    rows, cols, W, H = GRID_A
    r = demux(host, tmp_path, M.mux(SET_A, grid=GRID_A, tile_size=(64, 64), **GRID[name]))
    assert r["status"] == 0, r["message"]
    assert (r["codec"], r["grid"], r["rows"], r["cols"], r["w"], r["h"], r["orient"]) == (265, 1, rows, cols, W, H, 0)
    assert r["tiles"] == [M.expected_annexb(s) for s in SET_A]


def test_grid_shapes(host, tmp_path):
    for name, cols, rows, W, H in HR.CASES:
        r = demux(host, tmp_path, M.mux(list(HR.tiles(name))[:rows * cols], grid=(rows, cols, W, H)))
        assert (r["status"], r["rows"], r["cols"], r["w"], r["h"]) == (0, rows, cols, W, H), (name, r["message"])
        assert r["tiles"] == [M.expected_annexb(s) for s in HR.tiles(name)[:rows * cols]]


ROT = {0: 0, 1: 8, 2: 3, 3: 6}  # irot: angle x 90 degrees anticlockwise
MIR = {0: 2, 1: 4}              # imir: axis 0 vertical (left-right mirror), 1 horizontal


def composed(transforms):
    """the one orientation that equals the transforms applied in order, found on a plane with no symmetry"""
    p = np.arange(12).reshape(3, 4)
    q = p
    for kind, v in transforms:
        q = OR.orient_plane(q, ROT[v] if kind == "irot" else MIR[v])
    (o,) = [o for o in (0, 2, 3, 4, 5, 6, 7, 8) if OR.orient_plane(p, o).shape == q.shape and np.array_equal(OR.orient_plane(p, o), q)]
    return o


def test_orientation_in_ipma_order(host, tmp_path):
    seen = set()
    for a in range(4):
        for axis in (0, 1):
            for tr in ([("irot", a)], [("imir", axis)], [("irot", a), ("imir", axis)], [("imir", axis), ("irot", a)]):
                want = composed(tr)
                seen.add(want)
                for data in (M.mux([P11], transforms=tr), M.mux(SET_A, grid=GRID_A, transforms=tr, ipma_wide=True)):
                    r = demux(host, tmp_path, data)
                    assert r["status"] == 0 and r["orient"] == want, (tr, r["orient"], want)
    assert seen == {0, 2, 3, 4, 5, 6, 7, 8}
    assert composed([("irot", 1), ("imir", 0)]) != composed([("imir", 0), ("irot", 1)])  # the order matters


def test_compose_table(host):
    """heif_compose_orient over all pairs against numpy"""
    p = np.arange(12).reshape(3, 4)
    for a in range(9):
        for b in range(9):
            q = OR.orient_plane(OR.orient_plane(p, a), b)
            (want,) = [o for o in (0, 2, 3, 4, 5, 6, 7, 8) if OR.orient_plane(p, o).shape == q.shape and np.array_equal(OR.orient_plane(p, o), q)]
            assert int(subprocess.check_output([host, "compose", str(a), str(b)])) == want, (a, b)


def test_rejections(host, tmp_path):
    h264 = list(HR.tiles("h264"))
    whole = M.mux([P11])
    cases = [
        (whole[:len(whole) // 3], "HEIF: truncated or malformed box structure"),
        (whole[:len(whole) - 10], "HEIF: item data outside the file"),
        (M.mux([P11], no_pitm=True), "HEIF: no primary item"),
        (M.mux([P11], no_config=True), "HEIF: item has no decoder configuration"),
        (M.mux([P11], essential_unknown=True), "HEIF: essential property 'zzzz' unsupported"),
        (M.mux(SET_A, grid=GRID_A, drop_refs=1), "HEIF: grid references 3 items, needs 2 × 2"),
        (M.mux(h264, grid=(2, 2, 128, 128), tile_codec=264), "HEIF: grid of AVC tiles unsupported"),
        (M.mux(SET_A, grid=GRID_A, essential_unknown=True), "HEIF: essential property 'zzzz' unsupported"),
    ] + [(M.mux([P11], primary_type=t), f"HEIF: primary item type '{t.decode()}' unsupported") for t in (b"av01", b"iovl", b"iden", b"jpeg")]
    for data, message in cases:
        r = demux(host, tmp_path, data)
        assert r["heif"] == 1 and r["status"] < 0 and r["message"] == message, (r["status"], r["message"], message)
        assert r["tiles"] == []


def test_detection(host, tmp_path):
    def probe(data):
        path = str(tmp_path / "probe.bin")
        with open(path, "wb") as f:
            f.write(data)
        return int(subprocess.check_output([host, "probe", path]))

    good = M.mux([P11])
    assert probe(good) == 1 and probe(M.mux([A11], codec=264, brand=b"avci")) == 1
    assert probe(good[:16]) == 1 and probe(good[:15]) == 0
    assert probe(good.replace(b"heic", b"avif").replace(b"mif1", b"miaf")) == 0  # no brand of ours
    assert probe(b"\x00\x00\x00\x0e" + good[4:]) == 0 and probe(b"\x00\x00\x10\x04" + good[4:]) == 0  # size 14; 4100
    assert probe(b"\x00\x00\x00\x1a" + good[4:]) == 0  # no multiple of 4
    assert probe(good[:4] + b"styp" + good[8:]) == 0
    assert probe(P11) == 0 and probe(A11) == 0


def zero_width_iloc(entries, extent_count=0xFFFF, version=0):
    """ftyp + meta{hdlr, pitm, iloc}: every size nibble of the iloc 0, so an extent entry occupies no byte, and
    `entries` items of 6 bytes that each announce extent_count extents"""
    hdlr = M.fullbox(b"hdlr", 0, 0, struct.pack(">I4s", 0, b"pict") + b"\x00" * 13)
    pitm = M.fullbox(b"pitm", 0, 0, struct.pack(">H", 1))
    body = bytes([0, 0]) + struct.pack(">H", entries)
    for i in range(entries):
        body += struct.pack(">H", i + 1) + (struct.pack(">H", 0) if version else b"") + struct.pack(">HH", 0, extent_count)
    meta = M.fullbox(b"meta", 0, 0, hdlr + pitm + M.fullbox(b"iloc", version, 0, body))
    return M.box(b"ftyp", b"heic" + struct.pack(">I", 0) + b"mif1heic") + meta


def test_extent_counts_are_bounded_by_the_bytes_they_occupy(host, host_san, tmp_path):
    """An extent list whose entries have no width costs the file nothing per extent: 16384 items of 65535 extents fit
    in 98 KB and would ask for 16 GiB if the count were believed.  The demuxer must answer at once, inside 256 MiB
    (the whole process, program and libraries included); one zero-width extent, "the whole source", stays legal"""
    for entries, version in ((300, 0), (16384, 0), (16384, 1)):
        data = zero_width_iloc(entries, version=version)
        assert len(data) < 140000
        r = demux(host, tmp_path, data, limit_mib=256)
        assert r["status"] < 0 and r["message"] == "HEIF: truncated or malformed box structure", r
    for data in (zero_width_iloc(300), zero_width_iloc(16384, 2)):
        assert demux(host_san, tmp_path, data)["message"] == "HEIF: truncated or malformed box structure"
    # counts that fit their bytes are read: one zero-width extent per item, and then the file has no item type
    assert demux(host, tmp_path, zero_width_iloc(16384, 1), limit_mib=256)["message"] == "HEIF: no primary item"
    # a count larger than the bytes left in the box, with entries of real width
    whole = M.mux([P11], extents=2)
    off, _ = M.find_box(whole, b"meta")
    at = whole.index(b"iloc", off) + 4 + 4 + 2 + 2 + 2 + 2  # version/flags, nibbles, item_count, item_ID, data_reference_index
    assert whole[at:at + 2] == b"\x00\x02"
    r = demux(host, tmp_path, whole[:at] + b"\xff\xff" + whole[at + 2:], limit_mib=256)
    assert r["message"] == "HEIF: truncated or malformed box structure"


def _corpus(exe, tmp, data):
    path = str(tmp / "corpus.heic")
    with open(path, "wb") as f:
        f.write(data)
    off, n = M.find_box(data, b"meta")
    p = subprocess.run([exe, "corpus", path, str(off), str(n)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stdout[-500:], p.stderr[-3000:])
    w = p.stdout.split()
    cases, errors, sound = int(w[1]), int(w[3]), int(w[5])
    assert cases == len(data) + 3 * n and errors + sound == cases
    assert errors >= len(data) - 8 and sound > 0  # every truncation fails or is not HEIF; some mutations are harmless
    return cases


@pytest.mark.parametrize("which", ["single", "grid"])
def test_truncations_and_mutations(host, tmp_path, which):
    data = M.mux([B0], thumb=True, transforms=[("irot", 1)]) if which == "single" else M.mux(SET_A, grid=GRID_A, aux=True, transforms=[("imir", 0)])
    _corpus(host, tmp_path, data)


def test_corpus_under_sanitizers(host_san, tmp_path):
    """the same files, variants and corpus through the address + undefined-behaviour sanitizer build: clean"""
    for k in list(SINGLE.values()):
        assert demux(host_san, tmp_path, M.mux([P11], **k))["status"] == 0
    for k in list(GRID.values()):
        assert demux(host_san, tmp_path, M.mux(SET_A, grid=GRID_A, **k))["status"] == 0
    assert demux(host_san, tmp_path, M.mux(SET_A, grid=GRID_A, drop_refs=2))["status"] < 0
    _corpus(host_san, tmp_path, M.mux([B0], thumb=True, transforms=[("irot", 1)]))
    _corpus(host_san, tmp_path, M.mux(SET_A, grid=GRID_A, aux=True, transforms=[("imir", 0)]))
    _corpus(host_san, tmp_path, M.mux(SET_A, grid=GRID_A, iloc_version=2, construction=1, extents=2, ipma_wide=True, largesize=True))
