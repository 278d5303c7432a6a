"""The Annex-B scan against a byte-wise reference.

bitstream.cpp finds start codes and emulation-prevention bytes with memchr over the stretches that cannot hold one
(DESIGN.md §6); NAL bounds and unescaped bytes must be what a byte-at-a-time scan gives.  The reference below is that
scan, written here.  tests/annexb_scan/annexb_scan_case.cpp runs the library's functions on heap blocks of exactly
the input's size; it is built plain and with AddressSanitizer + UndefinedBehaviorSanitizer (host code with its own
main: the runtimes are linked into the program, nothing is preloaded, no GPU)."""
import os
import random
import struct
import subprocess
import zlib

import pytest

from conftest import PKG, ROOT

HOST = os.path.join(PKG, "csrc", "host")


def ref_split(d):
    """NAL units as (offset, length): the bytes after each 00 00 01 up to the next one, trailing zeros dropped."""
    out, i, start, n = [], 0, -1, len(d)

    def close(e):
        while e > start and d[e - 1] == 0:
            e -= 1
        out.append((start, e - start))

    while i + 2 < n:
        if d[i] == 0 and d[i + 1] == 0 and d[i + 2] == 1:
            if start >= 0:
                close(i)
            i += 3
            start = i
        else:
            i += 1
    if 0 <= start < n:
        close(n)
    return out


def ref_unescape(d):
    out, zeros = bytearray(), 0
    for b in d:
        if zeros >= 2 and b == 3:
            zeros = 0
            continue
        out.append(b)
        zeros = zeros + 1 if b == 0 else 0
    return bytes(out)


def ref_line(d):
    nals = ref_split(d)
    whole = ref_unescape(d)
    crc = 0
    for off, ln in nals:
        crc = zlib.crc32(ref_unescape(d[off:off + ln]), crc)
    return " ".join([str(len(nals))] + [f"{o},{ln}" for o, ln in nals] +
                    [str(len(whole)), f"{zlib.crc32(whole):08x}", f"{crc:08x}"])


def cases():
    c = [
        b"\x00\x00\x01\x40\x01\x0c",                              # 3-byte start code
        b"\x00\x00\x00\x01\x40\x01\x0c",                          # 4-byte start code
        b"\x00\x00\x00\x01\x67\x42\x00\x00\x01\x68\xce\x00\x00\x00\x01\x65\x88",  # both, back to back NALs
        b"\x00\x00\x01\x41\x9a\x00\x00\x01",                      # a start code in the last 3 bytes
        b"\x00\x00\x01\x41\x9a\x00\x00\x00\x01",
        b"\x00\x00\x01\x41\x00\x00\x03",                          # 00 00 03 ends the buffer
        b"\x00\x00\x01\x41\x00\x00\x03\x03",                      # 00 00 03 03
        b"\x00\x00\x01\x41\x00\x00\x03\x03\x00\x00\x03\x00\x00\x03\x01",
        b"\x00" * 40,                                             # runs of zeros
        b"\x00" * 19 + b"\x01" + b"\x00" * 23 + b"\x01\x25\x00\x00\x00\x00\x00",
        b"\x00\x00\x03" * 9,
        b"\x00\x00\x00\x03\x00\x00\x00\x03\x00",
        b"\x00\x00\x01\x00\x00\x01\x65",                          # an empty NAL
        b"\x00\x00\x01\x00\x00\x00\x01\x00\x00\x01",              # empty NALs only
        b"\x00\x00\x01",
        b"\x01\x00\x00\x01\x01\x00\x00\x01\x01",
        b"\x00\x01\x00\x01\x00\x00\x01\x03\x00\x03\x00\x00\x03",
    ]
    # lengths 0-17: a start code, an emulation-prevention sequence or a lone 01 / 03 at every offset, in a
    # buffer of FF and in one of zeros, so that each crosses every position of an 8- or 16-byte word
    for n in range(18):
        for fill in (0xFF, 0x00):
            c.append(bytes([fill]) * n)
            for pat in (b"\x00\x00\x01", b"\x00\x00\x03", b"\x00\x00\x00\x01", b"\x01", b"\x03", b"\x00\x00\x03\x03",
                        b"\x00\x00\x01\x00\x00\x03"):
                for at in range(0, n - len(pat) + 1):
                    b = bytearray([fill]) * n
                    b[at:at + len(pat)] = pat
                    c.append(bytes(b))
                    if at >= 3:  # behind a start code, so that the unescaped NAL payload is checked too
                        b[0:3] = b"\x00\x00\x01"
                        c.append(bytes(b))
    rng = random.Random(20261020)
    for _ in range(2000):
        c.append(bytes(rng.choice((0x00, 0x01, 0x02, 0x03, 0xFF)) for _ in range(rng.randint(0, 64))))
    return c


@pytest.fixture(scope="module")
def case_file(tmp_path_factory):
    cs = cases()
    path = tmp_path_factory.mktemp("annexb_scan") / "cases.bin"
    with open(path, "wb") as f:
        for d in cs:
            f.write(struct.pack("<I", len(d)) + d)
    return str(path), [ref_line(d) for d in cs]


def _build(tmp_path, flags):
    exe = str(tmp_path / "annexb_scan_case")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++11", "-O2", "-g", "-Wall"] + flags +
                          ["-I" + HOST, "-o", exe, os.path.join(ROOT, "tests", "annexb_scan", "annexb_scan_case.cpp"),
                           os.path.join(HOST, "bitstream.cpp")])
    return exe


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                                        "-static-libubsan"]], ids=["plain", "asan_ubsan"])
def test_scan_equals_the_bytewise_reference(tmp_path, case_file, flags):
    path, want = case_file
    assert len(want) > 2500
    out = subprocess.run([_build(tmp_path, flags), path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert out.returncode == 0, (out.stdout.decode()[-500:], out.stderr.decode()[-3000:])
    got = out.stdout.decode().splitlines()
    assert len(got) == len(want)
    bad = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, bad[:5]
