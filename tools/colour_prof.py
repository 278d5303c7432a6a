#!/usr/bin/env python3
"""Measure K3v, the colour stage: the scale stage's time (stats()["scale_ms"], HIP events around K3o / K3s / K3r / K3p /
K3v / K3u / K3b / K3c) of N x tests/golden/img01.h264 with [{..., "colour": source}], minus the same without the option
-- the median of five batches each after one warm-up batch, the two alternating -- against a device-to-device
hipMemcpyAsync of the plane bytes K3v writes for such a batch (stats()["colour_bytes"]; HIP events, best of 5).  The
outputs are 960 x 540 (scale 1: the wide class) with a range-only source (BT.601 limited) and a matrix source (BT.709
limited), and unscaled 1080p (the plain 8-bit class) with both.  Prints a markdown report.

  python3 tools/colour_prof.py --n 256 > profiles/colour_k3v.md

No GPU: fails (there is no CPU path)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from finish_prof import d2d_copy_ms  # noqa: E402  (the same yardstick as K3u's, K3c's and K3b's)
from rgb_prof import measure  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--threads", type=int, default=0)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "h264-h265-to-jpeg_amd"))
    import h2j
    if h2j.device_count() <= 0:
        raise SystemExit("no HIP device")
    with open(os.path.join(ROOT, "tests", "golden", "img01.h264"), "rb") as f:
        streams = [f.read()] * args.n
    eng = h2j.Engine(0, args.threads)
    print("# Colour (K3v): the conversion against a device-to-device copy\n")
    print(f"`tools/colour_prof.py --n {args.n}`: {args.n} x `tests/golden/img01.h264` (1920 x 1080) through synchronous")
    print("`transcode_multi`; `scale_ms` is the engine's HIP-event time of the stage between SAO and K4, summed over the")
    print("batch's chunks.  Five batches of each rendition list, alternating, after one warm-up batch of each; the copy is")
    print("one `hipMemcpyAsync` (device to device) of the plane bytes K3v writes for the batch (`colour_bytes`), best of 5.\n")
    for geo, what in (({"scale": 1}, "960 x 540, the wide class"), ({}, "1920 x 1080 unscaled, the plain 8-bit class")):
        for source, work in ((("bt601", "limited"), "range only"), (("bt709", "limited"), "matrix")):
            without, with_ = [dict(geo) or 0], [dict(geo, colour=source)]
            a, b = measure(eng, streams, with_, without, (1 << 20) * args.n)
            nbytes = int(eng.stats()["colour_bytes"])  # (the last batch measured is a converted one)
            ma, mb = statistics.median(a), statistics.median(b)
            copy = d2d_copy_ms(nbytes)
            k3v = mb - ma
            print("| renditions | scale_ms, five batches | median |")
            print("|---|---|---|")
            print(f"| `{without}` | {', '.join(f'{x:.3f}' for x in a)} | {ma:.3f} |")
            print(f"| `{with_}` | {', '.join(f'{x:.3f}' for x in b)} | {mb:.3f} |")
            print(f"\n{what}, {work}: K3v = {mb:.3f} - {ma:.3f} = **{k3v:.3f} ms** per {args.n} pictures ({nbytes / 1e6:.1f} MB written and as "
                  f"many read: {2 * nbytes / (k3v * 1e-3) / 1e9:.0f} GB/s); the copy of {nbytes / 1e6:.1f} MB: **{copy:.3f} ms**; "
                  f"K3v / copy = **{k3v / copy:.2f}**.\n")


if __name__ == "__main__":
    main()
