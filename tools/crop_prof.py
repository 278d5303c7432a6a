#!/usr/bin/env python3
"""Measure the scale stage on windows of 1080p pictures (crop and cover): K3s and K3p on a window whose
origin is load-aligned and on one whose origin is not (the shifted loads), and K3r for a cover thumbnail.

Two modes:

  run        transcode N pictures of tests/golden/bench (tiled) with each configuration of --configs,
             twice each (the second is reported), and print one JSON line per configuration.  Meant to
             run under the kernel tracer, in a run of its own, no counters:
               rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o crop -- \\
                   python3 tools/crop_prof.py run --n 1024 > DIR/run.jsonl
             H2J_LIB_DIR selects another build of the libraries (a build with the kernels from before the
             shifted loads runs the unaligned window on the single-sample path: the A/B of DESIGN.md).
  summarise  read one or more DIRs (kernel trace + run.jsonl each) and print a markdown summary: per
             configuration the scale-stage kernel, its time per N pictures and the bandwidth its
             algorithmic bytes imply.

Every configuration launches one scale-stage kernel per GPU chunk, so the trace's K3s / K3p / K3r
dispatches, in time order, are cut by the chunk counts of run.jsonl.

No GPU: `run` fails (there is no CPU path)."""
import argparse
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ALIGNED, SHIFTED = (416, 0, 1080, 1080), (420, 0, 1080, 1080)
CONFIGS = {
    "k3s1_aligned": [{"crop": ALIGNED, "scale": 1}],
    "k3s1_shifted": [{"crop": SHIFTED, "scale": 1}],
    "k3s2_aligned": [{"crop": ALIGNED, "scale": 2}],
    "k3s2_shifted": [{"crop": SHIFTED, "scale": 2}],
    "k3p12_aligned": [{"crop": ALIGNED, "scale": 1}, {"crop": ALIGNED, "scale": 2}],
    "k3p12_shifted": [{"crop": SHIFTED, "scale": 1}, {"crop": SHIFTED, "scale": 2}],
    "k3r_cover256": [{"cover": (256, 256)}],
}
SCALE_KERNELS = ("k3s_downscale", "k3p_pyramid", "k3r_resample")


def run(args):
    sys.path.insert(0, os.path.join(ROOT, "h264-h265-to-jpeg_amd"))
    import h2j
    paths = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", args.set, "*.h26?")))
    if not paths:
        raise SystemExit(f"no streams in tests/golden/{args.set}")
    base = [open(p, "rb").read() for p in paths]
    streams = [base[i % len(base)] for i in range(args.n)]
    eng = h2j.Engine(0, args.threads)
    for name in args.configs.split(","):
        rend = CONFIGS[name]
        for rep in range(2):
            outs = eng.transcode_multi(streams, rend)
            if any(o is None for row in outs for o in row):
                raise SystemExit(f"{name}: a rendition failed: {eng.error()}")
        st = eng.stats()
        print(json.dumps({"config": name, "n": args.n, "set": args.set, "lib_dir": os.environ.get("H2J_LIB_DIR", ""),
                          "jpeg_bytes": sum(len(o) for row in outs for o in row),
                          "stats": {key: round(st[key], 4) for key in ("scale_ms", "jpeg_ms", "entropy_ms", "total_ms",
                                                                       "frames", "renditions", "chunks")}}), flush=True)


def _col(row, *subs):
    for key in row:
        if all(s in key.lower() for s in subs):
            return key
    raise KeyError(subs)


def bytes_per_picture(name):
    """Algorithmic bytes of the scale stage per picture: the window's 8-bit samples read once, the outputs written."""
    src = 1.5 * 1080 * 1080
    if name.startswith("k3s1"):
        return src + src / 4
    if name.startswith("k3s2"):
        return src + src / 16
    if name.startswith("k3p12"):
        return src + src / 4 + src / 16
    return src + 1.5 * 256 * 256


def summarise(args):
    print("# Crop and cover: the scale stage on 1080 x 1080 windows of 1080p pictures\n")
    print("Kernel trace (`rocprofv3 --kernel-trace --stats`, a run of its own, no counters); every configuration ran")
    print("twice and the second batch is reported.  Window (416, 0, 1080, 1080) starts load-aligned, (420, 0, 1080, 1080)")
    print("4 bytes behind a boundary in luma and 2 in chroma: what cover 540 and cover 270 of a 1080p picture read.\n")
    print("| run | build | configuration | kernel | dispatches | ms per batch | bytes per picture | GB/s |")
    print("|---|---|---|---|---|---|---|---|")
    for d in args.dirs:
        runs = [json.loads(l) for l in open(os.path.join(d, "run.jsonl")) if l.startswith("{")]
        traces = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if not traces:
            raise SystemExit(f"no kernel trace under {d}")
        with open(traces[0]) as f:
            rows = list(csv.DictReader(f))
        name_c, t0_c, t1_c = _col(rows[0], "kernel_name"), _col(rows[0], "start_timestamp"), _col(rows[0], "end_timestamp")
        disp = sorted(((int(r[t0_c]), int(r[t1_c]), r[name_c]) for r in rows if any(s in r[name_c] for s in SCALE_KERNELS)))
        at = 0
        for r in runs:
            chunks = int(r["stats"]["chunks"])
            mine = disp[at + chunks:at + 2 * chunks]  # the second of the two batches
            at += 2 * chunks
            kernels = sorted({n.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0] for _, _, n in mine})
            ms = sum(t1 - t0 for t0, t1, _ in mine) / 1e6
            bpp = bytes_per_picture(r["config"])
            build = os.path.basename(r["lib_dir"].rstrip("/")) or "this build"
            print(f"| {os.path.basename(d.rstrip('/'))} | {build} | {r['config']} | {', '.join(kernels)} | {len(mine)} | {ms:.3f} | "
                  f"{bpp:.0f} | {bpp * r['n'] / (ms * 1e-3) / 1e9:.0f} |")
        if at != len(disp):
            print(f"\n(run {d}: {len(disp) - at} scale-stage dispatches not attributed)\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="mode", required=True)
    r = sub.add_parser("run")
    r.add_argument("--n", type=int, default=1024)
    r.add_argument("--configs", default=",".join(CONFIGS))
    r.add_argument("--set", default="bench")
    r.add_argument("--threads", type=int, default=0)
    s = sub.add_parser("summarise")
    s.add_argument("dirs", nargs="+")
    args = ap.parse_args()
    run(args) if args.mode == "run" else summarise(args)


if __name__ == "__main__":
    main()
