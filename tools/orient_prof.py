#!/usr/bin/env python3
"""Measure K3o, the orientation stage: a mirroring orientation (3) and a transposing one (6) on whole
pictures, against a device-to-device copy of the same bytes.

Two modes:

  run        transcode N pictures of tests/golden/<set> (tiled) through synchronous transcode_multi with one
             oriented rendition per configuration of --configs, twice each (the second is reported), then
             time a device-to-device hipMemcpyAsync of the bytes K3o moves for such a batch (HIP events,
             best of 5), and print one JSON line per configuration and one for the copy.  Meant to run
             under the kernel tracer, in a run of its own, no counters:
               rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o orient -- \\
                   python3 tools/orient_prof.py run --n 1024 > DIR/run.jsonl
             H2J_LIB_DIR selects another build of the libraries (e.g. one with -DH2J_K3O_PLAIN_ORDER: the
             dispatcher's own workgroup order, the A/B of DESIGN.md).
  summarise  read one or more DIRs (kernel trace + run.jsonl each) and print a markdown summary: per
             configuration the K3o kernel, its time per N pictures, the bandwidth its bytes imply and its
             ratio to the copy.

Bytes moved per picture: 2 x 1.5 W H sizeof(sample) -- every sample read once and written once.
Every configuration launches one K3o kernel per GPU chunk, so the trace's K3o dispatches, in time order, are
cut by the chunk counts of run.jsonl.

No GPU: `run` fails (there is no CPU path)."""
import argparse
import csv
import ctypes
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONFIGS = {"orient3": [{"orient": 3}], "orient6": [{"orient": 6}], "orient2": [{"orient": 2}], "orient4": [{"orient": 4}],
           "orient5": [{"orient": 5}], "orient8": [{"orient": 8}]}
K3O_KERNELS = ("k3o_mirror", "k3o_transpose")


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


def run(args):
    sys.path.insert(0, os.path.join(ROOT, "h264-h265-to-jpeg_amd"))
    import h2j
    paths = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", args.set, "*.h26?")))
    if not paths:
        raise SystemExit(f"no streams in tests/golden/{args.set}")
    base = [open(p, "rb").read() for p in paths]
    streams = [base[i % len(base)] for i in range(args.n)]
    eng = h2j.Engine(0, args.threads)
    y, u, v, size, mode, win, ro, so = eng.decode_multi4(base[0], [{"orient": 0}], 0)
    bd = eng.decode(base[0], 0)[3]
    w, h, pel = size[0], size[1], 2 if bd > 8 else 1
    per_picture = 1.5 * w * h * pel  # read once, written once
    for name in args.configs.split(","):
        rend = CONFIGS[name]
        for rep in range(2):
            outs = eng.transcode_multi(streams, rend)
            if any(o is None for row in outs for o in row):
                raise SystemExit(f"{name}: a rendition failed: {eng.error()}")
        st = eng.stats()
        print(json.dumps({"config": name, "n": args.n, "set": args.set, "lib_dir": os.environ.get("H2J_LIB_DIR", ""),
                          "w": w, "h": h, "pel": pel, "bytes_moved_per_picture": 2 * per_picture,
                          "stats": {key: round(st[key], 4) for key in ("scale_ms", "jpeg_ms", "sao_ms", "total_ms", "frames",
                                                                       "renditions", "chunks")}}), flush=True)
    ms = d2d_copy_ms(int(per_picture * args.n))
    print(json.dumps({"config": "d2d_copy", "n": args.n, "set": args.set, "w": w, "h": h, "pel": pel,
                      "bytes_moved_per_picture": 2 * per_picture, "ms": round(ms, 4)}), flush=True)


def _col(row, *subs):
    for key in row:
        if all(s in key.lower() for s in subs):
            return key
    raise KeyError(subs)


def summarise(args):
    print("# Orientation (K3o): whole pictures rotated and mirrored, against a device-to-device copy\n")
    print("Kernel trace (`rocprofv3 --kernel-trace --stats`, a run of its own, no counters); every configuration ran")
    print("twice through synchronous `transcode_multi` and the second batch is reported.  Bytes moved per picture are")
    print("2 x 1.5 W H sizeof(sample); the copy is one `hipMemcpyAsync` (device to device) of a batch's samples, timed")
    print("with HIP events in the same process, best of 5.\n")
    print("| run | build | set | configuration | kernel | dispatches | ms per batch | MB moved per picture | GB/s | time / copy |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for d in args.dirs:
        runs = [json.loads(l) for l in open(os.path.join(d, "run.jsonl")) if l.startswith("{")]
        traces = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if not traces:
            raise SystemExit(f"no kernel trace under {d}")
        with open(traces[0]) as f:
            rows = list(csv.DictReader(f))
        name_c, t0_c, t1_c = _col(rows[0], "kernel_name"), _col(rows[0], "start_timestamp"), _col(rows[0], "end_timestamp")
        disp = sorted(((int(r[t0_c]), int(r[t1_c]), r[name_c]) for r in rows if any(s in r[name_c] for s in K3O_KERNELS)))
        copy = next((r for r in runs if r["config"] == "d2d_copy"), None)
        at, times = 0, {}
        tag = os.path.basename(d.rstrip("/"))
        for r in runs:
            if r["config"] == "d2d_copy":
                continue
            chunks = int(r["stats"]["chunks"])
            mine = disp[at + chunks:at + 2 * chunks]  # the second of the two batches
            at += 2 * chunks
            kernels = sorted({n.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0] for _, _, n in mine})
            ms = sum(t1 - t0 for t0, t1, _ in mine) / 1e6
            times[r["config"]] = ms
            bpp = r["bytes_moved_per_picture"]
            build = os.path.basename(r["lib_dir"].rstrip("/")) or "this build"
            ratio = f"{ms / copy['ms']:.2f}" if copy else "-"
            print(f"| {tag} | {build} | {r['set']} | {r['config']} | {', '.join(kernels)} | {len(mine)} | {ms:.3f} | {bpp / 1e6:.2f} | "
                  f"{bpp * r['n'] / (ms * 1e-3) / 1e9:.0f} | {ratio} |")
        if copy:
            bpp = copy["bytes_moved_per_picture"]
            print(f"| {tag} | - | {copy['set']} | d2d_copy | hipMemcpyAsync | 1 | {copy['ms']:.3f} | {bpp / 1e6:.2f} | "
                  f"{bpp * copy['n'] / (copy['ms'] * 1e-3) / 1e9:.0f} | 1.00 |")
        if "orient3" in times and "orient6" in times:
            print(f"\n(run {tag}: transposing / mirroring time = {times['orient6'] / times['orient3']:.2f})\n")
        if at != len(disp):
            print(f"\n(run {tag}: {len(disp) - at} K3o dispatches not attributed)\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="mode", required=True)
    r = sub.add_parser("run")
    r.add_argument("--n", type=int, default=1024)
    r.add_argument("--configs", default="orient3,orient6")
    r.add_argument("--set", default="bench")
    r.add_argument("--threads", type=int, default=0)
    s = sub.add_parser("summarise")
    s.add_argument("dirs", nargs="+")
    args = ap.parse_args()
    run(args) if args.mode == "run" else summarise(args)


if __name__ == "__main__":
    main()
