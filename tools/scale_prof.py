#!/usr/bin/env python3
"""Measure the scaled-output stage (K3s) on a batch of 1080p HEVC pictures.

Two modes:

  run        transcode N pictures of tests/golden/bench (tiled) at each scale of --scales, twice
             each (the second is reported), and print one JSON line per scale with the engine's
             stage times.  Meant to run under the kernel tracer, in a run of its own:
               rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o scale -- \\
                   python3 tools/scale_prof.py run --n 1024 --scales 0,1,3 > DIR/run.jsonl
  summarise  read DIR's kernel trace and run.jsonl and print a markdown summary: per kernel and
             launch shape the dispatches and their time, K3s's time per N pictures and the
             bandwidth it implies -- (b S + S / 4^k) bytes per picture, S = 1.5 W H samples of b
             bytes -- beside K4a's, and the K4 + K5 stage times per scale.

No GPU: `run` fails (there is no CPU path)."""
import argparse
import collections
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(args):
    sys.path.insert(0, os.path.join(ROOT, "h264-h265-to-jpeg_amd"))
    import h2j
    paths = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", args.set, "*.h26?")))
    if not paths:
        raise SystemExit(f"no streams in tests/golden/{args.set}")
    base = [open(p, "rb").read() for p in paths]
    streams = [base[i % len(base)] for i in range(args.n)]
    eng = h2j.Engine(0, args.threads)
    for k in [int(x) for x in args.scales.split(",")]:
        for rep in range(2):
            outs = eng.transcode(streams, scale=k)
            if any(o is None for o in outs):
                raise SystemExit(f"scale {k}: a picture failed: {eng.error()}")
        st = eng.stats()
        print(json.dumps({"scale_log2": k, "n": args.n, "set": args.set, "jpeg_bytes": sum(len(o) for o in outs),
                          "stats": {key: round(st[key], 4) for key in (
                              "sao_ms", "scale_ms", "jpeg_ms", "entropy_ms", "d2h_ms", "assemble_ms", "total_ms",
                              "frames", "chunks", "payload_bytes", "payload_copied_bytes")}}), flush=True)


def _col(row, *subs):
    for key in row:
        if all(s in key.lower() for s in subs):
            return key
    raise KeyError(subs)


def summarise(args):
    runs = [json.loads(l) for l in open(os.path.join(args.dir, "run.jsonl")) if l.startswith("{")]
    traces = glob.glob(os.path.join(args.dir, "**", "*kernel_trace.csv"), recursive=True)
    if not traces:
        raise SystemExit(f"no kernel trace under {args.dir}")
    acc = collections.OrderedDict()
    with open(traces[0]) as f:
        rows = list(csv.DictReader(f))
    name_c, t0_c, t1_c = _col(rows[0], "kernel_name"), _col(rows[0], "start_timestamp"), _col(rows[0], "end_timestamp")
    gx_c, gy_c, wx_c = _col(rows[0], "grid_size_x"), _col(rows[0], "grid_size_y"), _col(rows[0], "workgroup_size_x")
    for r in rows:
        name = r[name_c].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        if not any(s in name for s in ("k3s_downscale", "k4a_variance", "k3_sao", "k4c_fdct_sym")):
            continue
        key = (name, int(r[gx_c]) // max(1, int(r[wx_c])), int(r[gy_c]))  # workgroups in x, pictures in y
        a = acc.setdefault(key, [0, 0.0])
        a[0] += 1
        a[1] += (int(r[t1_c]) - int(r[t0_c])) / 1e6
    n = runs[0]["n"]
    W, H = args.width, args.height
    S = 1.5 * W * H
    print(f"# Scaled output on {n} x {W}x{H} pictures of tests/golden/{runs[0]['set']}\n")
    print("Kernel trace (one run, no counters), dispatches grouped by kernel and launch shape; every scale ran twice,")
    print("so a batch of n pictures is half of each group's dispatches.\n")
    print("| kernel | workgroups x | pictures y | dispatches | total ms | ms per dispatch |")
    print("|---|---|---|---|---|---|")
    for (name, gx, gy), (cnt, ms) in acc.items():
        print(f"| {name} | {gx} | {gy} | {cnt} | {ms:.3f} | {ms / cnt:.4f} |")
    print()
    print("K3s per batch, and the bandwidth its algorithmic bytes imply (b S + S / 4^k per picture):\n")
    print("| kernel | ms per batch | bytes per picture | GB/s |")
    print("|---|---|---|---|")
    per = collections.OrderedDict()
    for (name, gx, gy), (cnt, ms) in acc.items():
        if "k3s_downscale" in name:
            p = per.setdefault(name, [0.0, 0])
            p[0] += ms
            p[1] += cnt * gy
    for name, (ms, pics) in per.items():
        k = int(name.rstrip(">").split(",")[-1])
        b = 2 if "short" in name else 1
        bpp = b * S + S / 4 ** k
        ms_batch = ms * n / pics
        print(f"| {name} | {ms_batch:.3f} | {bpp:.0f} | {bpp * n / (ms_batch * 1e-3) / 1e9:.0f} |")
    print()
    print("Stage times per batch from the engine's events (second of two batches per scale):\n")
    print("| scale_log2 | sao_ms | scale_ms | jpeg_ms (K4) | entropy_ms (K5) | K4 + K5 | d2h_ms | JPEG bytes |")
    print("|---|---|---|---|---|---|---|---|")
    for r in runs:
        s = r["stats"]
        print(f"| {r['scale_log2']} | {s['sao_ms']:.3f} | {s['scale_ms']:.3f} | {s['jpeg_ms']:.3f} | {s['entropy_ms']:.3f} | "
              f"{s['jpeg_ms'] + s['entropy_ms']:.3f} | {s['d2h_ms']:.3f} | {r['jpeg_bytes']} |")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="mode", required=True)
    r = sub.add_parser("run")
    r.add_argument("--n", type=int, default=1024)
    r.add_argument("--scales", default="0,1,3")
    r.add_argument("--set", default="bench")
    r.add_argument("--threads", type=int, default=0)
    s = sub.add_parser("summarise")
    s.add_argument("dir")
    s.add_argument("--width", type=int, default=1920)
    s.add_argument("--height", type=int, default=1080)
    args = ap.parse_args()
    run(args) if args.mode == "run" else summarise(args)


if __name__ == "__main__":
    main()
