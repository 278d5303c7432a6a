#!/usr/bin/env python3
"""Measure K3c, the RGB output stage: the scale stage's time (stats()["scale_ms"], HIP events around K3o / K3s / K3r /
K3p / K3u / K3c) of N x tests/golden/img01.h264 with [{"scale": 1, "format": "rgb"}], minus the same with
[{"scale": 1}] -- the median of five batches each after one warm-up batch, the two alternating -- against a
device-to-device hipMemcpyAsync of the pixel bytes K3c writes for such a batch (HIP events, best of 5).  Prints a
markdown report.  --unscaled adds the same for [{"format": "rgb"}] against [0] (the plain sample path); --planar
measures "rgb_planar" instead.

  python3 tools/rgb_prof.py --n 256 --unscaled > profiles/rgb_k3c.md

No GPU: fails (there is no CPU path)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from finish_prof import d2d_copy_ms  # noqa: E402  (the same yardstick as K3u's)


def measure(eng, streams, with_, without, cap, runs=5):
    """scale_ms of `runs` batches of each rendition list, alternating, after one warm-up batch of each."""
    ms = {0: [], 1: []}
    for rep in range(runs + 1):
        for k, rend in enumerate((without, with_)):
            outs = eng.transcode_multi(streams, rend, out_cap=cap)
            if any(o is None for row in outs for o in row):
                raise SystemExit(f"{rend}: a rendition failed: {eng.error()}")
            del outs
            if rep:
                ms[k].append(eng.stats()["scale_ms"])
    return ms[0], ms[1]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--threads", type=int, default=0)
    ap.add_argument("--unscaled", action="store_true")
    ap.add_argument("--planar", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "h264-h265-to-jpeg_amd"))
    import h2j
    if h2j.device_count() <= 0:
        raise SystemExit("no HIP device")
    with open(os.path.join(ROOT, "tests", "golden", "img01.h264"), "rb") as f:
        streams = [f.read()] * args.n
    eng = h2j.Engine(0, args.threads)
    fmt = "rgb_planar" if args.planar else "rgb"
    flags = f"{' --unscaled' if args.unscaled else ''}{' --planar' if args.planar else ''}"
    print("# RGB output (K3c): the conversion against a device-to-device copy\n")
    print(f"`tools/rgb_prof.py --n {args.n}{flags}`: {args.n} x `tests/golden/img01.h264` (1920 x 1080) through synchronous")
    print("`transcode_multi`; `scale_ms` is the engine's HIP-event time of the stage between SAO and K4, summed over the")
    print("batch's chunks.  Five batches of each rendition list, alternating, after one warm-up batch of each; the copy is")
    print("one `hipMemcpyAsync` (device to device) of the bytes K3c writes for the batch, best of 5.\n")
    print("| renditions | scale_ms, five batches | median |")
    print("|---|---|---|")
    rows = [("scale 1 (the hot class)", [{"scale": 1}], [{"scale": 1, "format": fmt}])]
    if args.unscaled:
        rows.append(("unscaled (the plain class)", [0], [{"format": fmt}]))
    for label, without, with_ in rows:
        size = eng.decode_multi5(streams[0], without, 0)[3]
        nbytes = 3 * size[0] * size[1] * args.n
        a, b = measure(eng, streams, with_, without, nbytes + (1 << 20) * args.n)
        ma, mb = statistics.median(a), statistics.median(b)
        copy = d2d_copy_ms(nbytes)
        print(f"| `{without}` | {', '.join(f'{x:.3f}' for x in a)} | {ma:.3f} |")
        print(f"| `{with_}` | {', '.join(f'{x:.3f}' for x in b)} | {mb:.3f} |")
        k3c = mb - ma
        print(f"\n{label}: K3c = {mb:.3f} - {ma:.3f} = **{k3c:.3f} ms** per {args.n} pictures of {size[0]} x {size[1]} "
              f"({nbytes / 1e6:.1f} MB written, half as many read: {1.5 * nbytes / (k3c * 1e-3) / 1e9:.0f} GB/s); the copy of {nbytes / 1e6:.1f} MB: "
              f"**{copy:.3f} ms**; K3c / copy = **{k3c / copy:.2f}**.\n")
        if label != rows[-1][0]:
            print("| renditions | scale_ms, five batches | median |")
            print("|---|---|---|")


if __name__ == "__main__":
    main()
