#!/usr/bin/env python3
"""Measure K3u, the finishing stage's unsharp mask: the scale stage's time (stats()["scale_ms"], HIP events around
K3o / K3s / K3r / K3p / K3u) of N x tests/golden/img01.h264 with [{"scale": 1, "sharpen": 16}], minus the same with
[{"scale": 1}] -- the median of five batches each after one warm-up batch, the two alternating -- against a
device-to-device hipMemcpyAsync of the plane bytes K3u writes for such a batch (HIP events, best of 5).  Prints a
markdown report.  --unscaled adds the same for [{"sharpen": 16}] against [0] (the plain sample path).

  python3 tools/finish_prof.py --n 256 > profiles/finish_k3u.md

No GPU: fails (there is no CPU path)."""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def d2d_copy_ms(nbytes, reps=5):
    """Best-of-reps milliseconds of one device-to-device hipMemcpyAsync of nbytes (HIP events on the null stream)."""
    hip = ctypes.CDLL("libamdhip64.so")
    src, dst, e0, e1 = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()

    def ok(rc, what):
        if rc != 0:
            raise SystemExit(f"{what} failed ({rc})")

    ok(hip.hipMalloc(ctypes.byref(src), ctypes.c_size_t(nbytes)), "hipMalloc")
    ok(hip.hipMalloc(ctypes.byref(dst), ctypes.c_size_t(nbytes)), "hipMalloc")
    ok(hip.hipMemset(src, 1, ctypes.c_size_t(nbytes)), "hipMemset")
    ok(hip.hipEventCreate(ctypes.byref(e0)), "hipEventCreate")
    ok(hip.hipEventCreate(ctypes.byref(e1)), "hipEventCreate")
    best = None
    for rep in range(reps + 1):  # the first is a warm-up
        ok(hip.hipEventRecord(e0, None), "hipEventRecord")
        ok(hip.hipMemcpyAsync(dst, src, ctypes.c_size_t(nbytes), 3, None), "hipMemcpyAsync")  # 3: hipMemcpyDeviceToDevice
        ok(hip.hipEventRecord(e1, None), "hipEventRecord")
        ok(hip.hipEventSynchronize(e1), "hipEventSynchronize")
        ms = ctypes.c_float(0)
        ok(hip.hipEventElapsedTime(ctypes.byref(ms), e0, e1), "hipEventElapsedTime")
        if rep:
            best = ms.value if best is None else min(best, ms.value)
    for p in (src, dst):
        hip.hipFree(p)
    return best


def measure(eng, streams, with_, without, runs=5):
    """scale_ms of `runs` batches of each rendition list, alternating, after one warm-up batch of each."""
    ms = {0: [], 1: []}
    for rep in range(runs + 1):
        for k, rend in enumerate((without, with_)):
            outs = eng.transcode_multi(streams, rend)
            if any(o is None for row in outs for o in row):
                raise SystemExit(f"{rend}: a rendition failed: {eng.error()}")
            if rep:
                ms[k].append(eng.stats()["scale_ms"])
    return ms[0], ms[1]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--threads", type=int, default=0)
    ap.add_argument("--unscaled", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "h264-h265-to-jpeg_amd"))
    import h2j
    if h2j.device_count() <= 0:
        raise SystemExit("no HIP device")
    with open(os.path.join(ROOT, "tests", "golden", "img01.h264"), "rb") as f:
        streams = [f.read()] * args.n
    eng = h2j.Engine(0, args.threads)
    print("# Finishing (K3u): the unsharp mask against a device-to-device copy\n")
    print(f"`tools/finish_prof.py --n {args.n}{' --unscaled' if args.unscaled else ''}`: {args.n} x `tests/golden/img01.h264` (1920 x 1080) through synchronous")
    print("`transcode_multi`; `scale_ms` is the engine's HIP-event time of the stage between SAO and K4, summed over the")
    print("batch's chunks.  Five batches of each rendition list, alternating, after one warm-up batch of each; the copy is")
    print("one `hipMemcpyAsync` (device to device) of the bytes K3u writes for the batch, best of 5.\n")
    print("| renditions | scale_ms, five batches | median |")
    print("|---|---|---|")
    rows = [("scale 1", [{"scale": 1}], [{"scale": 1, "sharpen": 16}])]
    if args.unscaled:
        rows.append(("unscaled", [0], [{"sharpen": 16}]))
    for label, without, with_ in rows:
        size = eng.decode_multi5(streams[0], with_, 0)[3]
        nbytes = int(1.5 * size[0] * size[1]) * args.n
        a, b = measure(eng, streams, with_, without)
        ma, mb = statistics.median(a), statistics.median(b)
        copy = d2d_copy_ms(nbytes)
        print(f"| `{without}` | {', '.join(f'{x:.3f}' for x in a)} | {ma:.3f} |")
        print(f"| `{with_}` | {', '.join(f'{x:.3f}' for x in b)} | {mb:.3f} |")
        k3u = mb - ma
        print(f"\n{label}: K3u = {mb:.3f} - {ma:.3f} = **{k3u:.3f} ms** per {args.n} pictures of {size[0]} x {size[1]} "
              f"({nbytes / 1e6:.1f} MB written, as many read: {2 * nbytes / (k3u * 1e-3) / 1e9:.0f} GB/s); the copy of {nbytes / 1e6:.1f} MB: "
              f"**{copy:.3f} ms**; K3u / copy = **{k3u / copy:.2f}**.\n")
        if label != rows[-1][0]:
            print("| renditions | scale_ms, five batches | median |")
            print("|---|---|---|")


if __name__ == "__main__":
    main()
