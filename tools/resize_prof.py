#!/usr/bin/env python3
"""Measure the exact-size-output kernel (K3r) beside K3s on a batch of 1080p HEVC pictures.

Two modes:

  run        transcode N pictures of tests/golden/bench (tiled) in each mode of --modes
             (`fit:WxH`, `scale:K`), twice each (the second is reported), and print one JSON line
             per mode with the engine's stage times.  Meant to run under the kernel tracer, in a
             run of its own with no counters:
               rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o resize -- \\
                   python3 tools/resize_prof.py run --n 1024 > DIR/run.jsonl
  summarise  read DIR's kernel trace and run.jsonl and print a markdown summary: per kernel and
             launch shape the dispatches and their time, K3r's and K3s's time per N pictures and
             the bandwidth their algorithmic bytes imply -- (b S + S_o) bytes per picture, S =
             1.5 W H source samples of b bytes, S_o = 1.5 W_o H_o output bytes -- and the stage
             times per mode.

The dispatches of a mode are told apart by their grid width (workgroups per picture), which
differs between the modes of the default list.  No GPU: `run` fails (there is no CPU path)."""
import argparse
import collections
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parse_mode(m):
    kind, val = m.split(":")
    if kind == "fit":
        w, h = val.split("x")
        return {"fit": (int(w), int(h))}
    return {"scale": int(val)}


def run(args):
    sys.path.insert(0, os.path.join(ROOT, "h264-h265-to-jpeg_amd"))
    import h2j
    paths = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", args.set, "*.h26?")))
    if not paths:
        raise SystemExit(f"no streams in tests/golden/{args.set}")
    base = [open(p, "rb").read() for p in paths]
    streams = [base[i % len(base)] for i in range(args.n)]
    eng = h2j.Engine(0, args.threads)
    for mode in args.modes.split(","):
        kw = parse_mode(mode)
        for rep in range(2):
            outs = eng.transcode(streams, **kw)
            if any(o is None for o in outs):
                raise SystemExit(f"{mode}: a picture failed: {eng.error()}")
        st = eng.stats()
        out_size = h2j.fit_size(args.width, args.height, kw["fit"]) if "fit" in kw else \
            tuple(2 * -(-d // (2 << kw["scale"])) if kw["scale"] else d for d in (args.width, args.height))
        print(json.dumps({"mode": mode, "n": args.n, "set": args.set, "out_w": out_size[0], "out_h": out_size[1],
                          "src_w": args.width, "src_h": args.height, "jpeg_bytes": sum(len(o) for o in outs),
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
        if not any(s in name for s in ("k3r_resample", "k3s_downscale", "k4a_variance", "k4c_fdct_sym")):
            continue
        key = (name, int(r[gx_c]) // max(1, int(r[wx_c])), int(r[gy_c]))  # workgroups in x, pictures in y
        a = acc.setdefault(key, [0, 0.0])
        a[0] += 1
        a[1] += (int(r[t1_c]) - int(r[t0_c])) / 1e6
    n = runs[0]["n"]
    W, H = runs[0]["src_w"], runs[0]["src_h"]
    S = 1.5 * W * H
    print(f"# Exact-size output on {n} x {W}x{H} pictures of tests/golden/{runs[0]['set']}\n")
    print("Kernel trace (one run, no counters), dispatches grouped by kernel and launch shape; every mode ran twice,")
    print("so a batch of n pictures is half of each group's dispatches.\n")
    print("| kernel | workgroups x | pictures y | dispatches | total ms | ms per dispatch |")
    print("|---|---|---|---|---|---|")
    for (name, gx, gy), (cnt, ms) in acc.items():
        print(f"| {name} | {gx} | {gy} | {cnt} | {ms:.3f} | {ms / cnt:.4f} |")
    print()

    def k3r_tiles(w, h):  # include/h2j_gpu.h h2j_k3r_tiles
        pt = lambda a, b: ((((a + 3) >> 2) + 63) >> 6) * ((b + 31) >> 5)
        return pt(w, h) + 2 * pt(w // 2, h // 2)

    def k3s_tiles(w, h):  # include/h2j_gpu.h h2j_k3s_tiles
        pt = lambda a, b: ((((a + 3) >> 2) + 63) >> 6) * ((b + 3) >> 2)
        return pt(w, h) + 2 * pt(w // 2, h // 2)

    print("K3r and K3s per batch, and the bandwidth their algorithmic bytes imply (b S + S_o per picture):\n")
    print("| mode | output | kernel | ms per batch | bytes per picture | GB/s |")
    print("|---|---|---|---|---|---|")
    rates = {}
    for r in runs:
        ow, oh = r["out_w"], r["out_h"]
        if (ow, oh) == (W, H):
            continue
        is_fit = r["mode"].startswith("fit")
        want, tiles = ("k3r_resample", k3r_tiles(ow, oh)) if is_fit else ("k3s_downscale", k3s_tiles(ow, oh))
        ms, pics, kname = 0.0, 0, ""
        for (name, gx, gy), (cnt, t) in acc.items():
            if want in name and gx == tiles:
                ms += t
                pics += cnt * gy
                kname = name
        if not pics:
            continue
        bpp = S + 1.5 * ow * oh
        ms_batch = ms * n / pics
        rates[r["mode"]] = bpp * n / (ms_batch * 1e-3) / 1e9
        print(f"| {r['mode']} | {ow}x{oh} | {kname} | {ms_batch:.3f} | {bpp:.0f} | {rates[r['mode']]:.0f} |")
    print()
    if "scale:1" in rates:
        for m, v in rates.items():
            if m.startswith("fit"):
                print(f"K3r at {m}: {v / rates['scale:1']:.2f} of K3s's k = 1 rate in this run.")
        print()
    print("Stage times per batch from the engine's events (second of two batches per mode):\n")
    print("| mode | sao_ms | scale_ms | jpeg_ms (K4) | entropy_ms (K5) | K4 + K5 | d2h_ms | JPEG bytes |")
    print("|---|---|---|---|---|---|---|---|")
    for r in runs:
        s = r["stats"]
        print(f"| {r['mode']} | {s['sao_ms']:.3f} | {s['scale_ms']:.3f} | {s['jpeg_ms']:.3f} | {s['entropy_ms']:.3f} | "
              f"{s['jpeg_ms'] + s['entropy_ms']:.3f} | {s['d2h_ms']:.3f} | {r['jpeg_bytes']} |")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="mode", required=True)
    r = sub.add_parser("run")
    r.add_argument("--n", type=int, default=1024)
    r.add_argument("--modes", default="scale:0,scale:1,fit:1280x720,fit:512x512")
    r.add_argument("--set", default="bench")
    r.add_argument("--threads", type=int, default=0)
    r.add_argument("--width", type=int, default=1920)
    r.add_argument("--height", type=int, default=1080)
    s = sub.add_parser("summarise")
    s.add_argument("dir")
    args = ap.parse_args()
    run(args) if args.mode == "run" else summarise(args)


if __name__ == "__main__":
    main()
