#!/usr/bin/env python3
"""Measure K3b, the padding stage: the scale stage's time (stats()["scale_ms"], HIP events around K3o / K3s / K3r / K3p /
K3u / K3b / K3c) of N x tests/golden/img01.h264 with [{"fit": box, "pad": colour}], minus the same with [{"fit": box}]
-- the median of five batches each after one warm-up batch, the two alternating -- against a device-to-device
hipMemcpyAsync of the canvas bytes K3b writes for such a batch (stats()["pad_bytes"]; HIP events, best of 5).  The boxes
are 640 x 640 (the detector letterbox) and 224 x 224.  Prints a markdown report.

  python3 tools/pad_prof.py --n 256 > profiles/pad_k3b.md

No GPU: fails (there is no CPU path)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from finish_prof import d2d_copy_ms  # noqa: E402  (the same yardstick as K3u's and K3c's)
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
    print("# Padded output (K3b): the padding against a device-to-device copy\n")
    print(f"`tools/pad_prof.py --n {args.n}`: {args.n} x `tests/golden/img01.h264` (1920 x 1080) through synchronous")
    print("`transcode_multi`; `scale_ms` is the engine's HIP-event time of the stage between SAO and K4, summed over the")
    print("batch's chunks.  Five batches of each rendition list, alternating, after one warm-up batch of each; the copy is")
    print("one `hipMemcpyAsync` (device to device) of the canvas bytes K3b writes for the batch (`pad_bytes`), best of 5.\n")
    for box in ((640, 640), (224, 224)):
        without, with_ = [{"fit": box}], [{"fit": box, "pad": (114, 114, 114)}]
        r = eng.decode_multi7(streams[0], with_, 0)
        a, b = measure(eng, streams, with_, without, (1 << 20) * args.n)
        nbytes = int(eng.stats()["pad_bytes"])  # (the last batch measured is a padded one)
        ma, mb = statistics.median(a), statistics.median(b)
        copy = d2d_copy_ms(nbytes)
        k3b = mb - ma
        pic = r[11][2] * r[11][3] * 3 // 2
        print("| renditions | scale_ms, five batches | median |")
        print("|---|---|---|")
        print(f"| `{without}` | {', '.join(f'{x:.3f}' for x in a)} | {ma:.3f} |")
        print(f"| `{with_}` | {', '.join(f'{x:.3f}' for x in b)} | {mb:.3f} |")
        print(f"\n{box[0]} x {box[1]}: the picture part is {r[11][2]} x {r[11][3]} at ({r[11][0]}, {r[11][1]}): {100.0 * (1 - pic * args.n / nbytes):.0f} % of the "
              f"canvas bytes are fill.  K3b = {mb:.3f} - {ma:.3f} = **{k3b:.3f} ms** per {args.n} canvases ({nbytes / 1e6:.1f} MB written, "
              f"{pic * args.n / 1e6:.1f} MB read: {(nbytes + pic * args.n) / (k3b * 1e-3) / 1e9:.0f} GB/s); the copy of {nbytes / 1e6:.1f} MB: "
              f"**{copy:.3f} ms**; K3b / copy = **{k3b / copy:.2f}**.\n")


if __name__ == "__main__":
    main()
