#!/usr/bin/env python3
"""Measure renditions (several JPEGs of one decoded picture) on 1024 x 1080p 8-bit pictures of
tests/golden/bench.

Driver modes start every GPU step as a child process under its own `timeout` and stop at the first
step that fails:

  k3p DIR      one `rocprofv3 --kernel-trace --stats` run (no counters) of the `k3p-run` step: K3p for
               the levels (1, 2, 3) and the three K3s launches for the same pictures in one process;
               then prints the markdown summary of DIR's trace.
  e2e DIR      wall time of (a) transcode_multi with [0, 3] and [0, 1, 2, 3], (b) the same outputs
               asked for as a repeated stream list with scale=, on this build and on --parent-lib (an
               older build without the multi entry points, selected with H2J_LIB_DIR), (c) the plain
               unscaled call; every case a process of its own, the whole list run --passes times in
               alternation; then prints the markdown summary.

Steps (what the children run): k3p-run, case.  No GPU: they fail (there is no CPU path)."""
import argparse
import collections
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["plain", "multi03", "multi0123", "old03", "old0123"]
SETS = {"03": [0, 3], "0123": [0, 1, 2, 3]}


def _engine(args):
    sys.path.insert(0, os.path.join(ROOT, "h264-h265-to-jpeg_amd"))
    import h2j
    paths = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", args.set, "*.h26?")))
    if not paths:
        raise SystemExit(f"no streams in tests/golden/{args.set}")
    base = [open(p, "rb").read() for p in paths]
    return h2j.Engine(0, args.threads), [base[i % len(base)] for i in range(args.n)]


def k3p_run(args):
    eng, streams = _engine(args)
    keys = ("sao_ms", "scale_ms", "jpeg_ms", "entropy_ms", "total_ms", "frames", "renditions", "parsed")
    for rep in range(2):
        outs = eng.transcode_multi(streams, [1, 2, 3])
        if any(o is None for row in outs for o in row):
            raise SystemExit(f"multi: a rendition failed: {eng.error()}")
    st = eng.stats()
    print(json.dumps({"case": "multi123", "n": args.n, "set": args.set, "stats": {k: round(st[k], 4) for k in keys}}), flush=True)
    for k in (1, 2, 3):
        for rep in range(2):
            single = eng.transcode(streams, scale=k)
        if single != [row[k - 1] for row in outs]:
            raise SystemExit(f"scale {k}: K3s and K3p outputs differ")
        st = eng.stats()
        print(json.dumps({"case": f"scale{k}", "n": args.n, "set": args.set, "stats": {k2: round(st[k2], 4) for k2 in keys}}), flush=True)


def case(args):
    eng, streams = _engine(args)
    name = args.case
    rend = SETS.get(name.replace("multi", "").replace("old", ""))

    def once():
        if name == "plain":
            return eng.transcode(streams)
        if name.startswith("multi"):
            return eng.transcode_multi(streams, rend)
        return eng.transcode(streams * len(rend), scale=[k for k in rend for _ in streams])

    once()  # warm-up: buffers, payload estimate
    ms, eng_ms = [], []
    for rep in range(args.reps):
        t0 = time.perf_counter()
        outs = once()
        ms.append((time.perf_counter() - t0) * 1e3)
        eng_ms.append(eng.stats()["total_ms"])  # the engine's own wall time: submission to the last JPEG written
    flat = [o for row in outs for o in (row if isinstance(row, list) else [row])]
    if any(o is None for o in flat):
        raise SystemExit(f"{name}: an output failed: {eng.error()}")
    st = eng.stats()
    print(json.dumps({"case": name, "lib": os.environ.get("H2J_LIB_DIR", ""), "n": args.n, "outputs": len(flat),
                      "jpeg_bytes": sum(len(o) for o in flat), "wall_ms": [round(x, 1) for x in ms], "engine_ms": [round(x, 1) for x in eng_ms],
                      "parse_run_ms": round(st["parse_run_ms"], 1), "parsed": st.get("parsed", 0),
                      "scale_ms": round(st["scale_ms"], 3), "jpeg_ms": round(st["jpeg_ms"], 3),
                      "entropy_ms": round(st["entropy_ms"], 3), "assemble_ms": round(st["assemble_ms"], 1)}), flush=True)


def _step(cmd, limit, out_path, env=None):
    """One GPU step: a child under its own time limit; its stdout is appended to out_path."""
    full = ["timeout", "-k", "10", str(limit)] + cmd
    with open(out_path, "a") as f:
        rc = subprocess.call(full, stdout=f, env=env)
    if rc != 0:
        raise SystemExit(f"step failed ({rc}): {' '.join(cmd)}")


def _common(args):
    return ["--n", str(args.n), "--set", args.set, "--threads", str(args.threads)]


def k3p(args):
    os.makedirs(args.dir, exist_ok=True)
    run = os.path.join(args.dir, "run.jsonl")
    open(run, "w").close()
    _step(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", args.dir, "-o", "renditions", "--",
           sys.executable, os.path.abspath(__file__), "k3p-run"] + _common(args), args.limit, run)
    summarise_k3p(args)


def e2e(args):
    os.makedirs(args.dir, exist_ok=True)
    run = os.path.join(args.dir, "e2e.jsonl")
    open(run, "w").close()
    for p in range(args.passes):
        for name in CASES:
            libs = [None] + ([args.parent_lib] if args.parent_lib and name.startswith("old") else [])
            for lib in libs:
                env = dict(os.environ)
                if lib:
                    env["H2J_LIB_DIR"] = os.path.abspath(lib)
                _step([sys.executable, os.path.abspath(__file__), "case", "--case", name, "--reps", str(args.reps)] + _common(args),
                      args.limit, run, env)
    summarise_e2e(args)


def _col(row, *subs):
    for key in row:
        if all(s in key.lower() for s in subs):
            return key
    raise KeyError(subs)


def summarise_k3p(args):
    runs = [json.loads(l) for l in open(os.path.join(args.dir, "run.jsonl")) if l.startswith("{")]
    traces = glob.glob(os.path.join(args.dir, "**", "*kernel_trace.csv"), recursive=True)
    if not traces:
        raise SystemExit(f"no kernel trace under {args.dir}")
    with open(traces[0]) as f:
        rows = list(csv.DictReader(f))
    name_c, t0_c, t1_c = _col(rows[0], "kernel_name"), _col(rows[0], "start_timestamp"), _col(rows[0], "end_timestamp")
    gx_c, gy_c, wx_c = _col(rows[0], "grid_size_x"), _col(rows[0], "grid_size_y"), _col(rows[0], "workgroup_size_x")
    acc = collections.OrderedDict()
    for r in rows:
        name = r[name_c].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        if not any(s in name for s in ("k3p_pyramid", "k3s_downscale")):
            continue
        key = (name, int(r[gx_c]) // max(1, int(r[wx_c])), int(r[gy_c]))
        acc.setdefault(key, []).append((int(r[t1_c]) - int(r[t0_c])) / 1e6)
    n = runs[0]["n"]
    S = 1.5 * args.width * args.height
    print(f"# K3p against the three K3s launches it replaces, {n} x {args.width}x{args.height} pictures of tests/golden/{runs[0]['set']}\n")
    print("One `rocprofv3 --kernel-trace --stats` run without counters; one process ran `transcode_multi` with the levels")
    print("(1, 2, 3) twice, then `transcode` at scale 1, 2 and 3 twice each, on the same pictures.  Dispatches grouped")
    print("by kernel and launch shape (workgroups in x, pictures in y).\n")
    print("| kernel | workgroups x | pictures y | dispatches | median ms | min ms | max ms |")
    print("|---|---|---|---|---|---|---|")
    per = collections.OrderedDict()
    for (name, gx, gy), ms in acc.items():
        print(f"| {name} | {gx} | {gy} | {len(ms)} | {statistics.median(ms):.4f} | {min(ms):.4f} | {max(ms):.4f} |")
        p = per.setdefault(name, [0.0, 0])
        p[0] += sum(ms)
        p[1] += len(ms) * gy
    print("\nPer batch of n pictures, and the bandwidth the algorithmic bytes imply (S = 1.5 W H):\n")
    print("| kernel | ms per batch | bytes per picture | GB/s |")
    print("|---|---|---|---|")
    k3s_sum = 0.0
    k3p_ms = None
    for name, (ms, pics) in per.items():
        ms_batch = ms * n / pics
        if "k3p" in name:
            bpp = S + S / 4 + S / 16 + S / 64
            k3p_ms = ms_batch
        else:
            k = int(name.rstrip(">").split(",")[-1])
            bpp = S + S / 4 ** k
            k3s_sum += ms_batch
        print(f"| {name} | {ms_batch:.3f} | {bpp:.0f} | {bpp * n / (ms_batch * 1e-3) / 1e9:.0f} |")
    if k3p_ms is not None and k3s_sum > 0:
        print(f"\nK3p {k3p_ms:.3f} ms against {k3s_sum:.3f} ms for the three K3s launches: {k3s_sum / k3p_ms:.2f}x.\n")
    print("Stage times per batch from the engine's events (second of two batches per case):\n")
    print("| case | scale_ms | jpeg_ms (K4) | entropy_ms (K5) | frames | renditions | parsed |")
    print("|---|---|---|---|---|---|---|")
    for r in runs:
        s = r["stats"]
        print(f"| {r['case']} | {s['scale_ms']:.3f} | {s['jpeg_ms']:.3f} | {s['entropy_ms']:.3f} | {s['frames']:.0f} | "
              f"{s['renditions']:.0f} | {s['parsed']:.0f} |")


def summarise_e2e(args):
    runs = [json.loads(l) for l in open(os.path.join(args.dir, "e2e.jsonl")) if l.startswith("{")]
    groups = collections.OrderedDict()
    for r in runs:
        groups.setdefault((r["case"], "parent" if r["lib"] else "this"), []).append(r)
    n = runs[0]["n"]
    print(f"# Renditions end to end, {n} x 1080p pictures of tests/golden/bench, one box\n")
    print("Time of one call in ms; every case a process of its own (one warm-up call, then the timed calls), the list")
    print("of cases run in alternation.  engine: the engine's `total_ms`, submission to the last JPEG written (median,")
    print("min .. max); python: the wall time of the h2j.py call around it, which adds the ctypes arrays, the output")
    print("buffer and the bytes objects of every output.  (a) multi: `transcode_multi`; (b) old: the same outputs as a")
    print("repeated stream list with `scale=`, on this build and on the parent commit's; (c) plain: the unscaled call.\n")
    print("| case | build | outputs | calls | engine ms | engine min .. max | python ms | pictures parsed | parse_run_ms | scale_ms | jpeg_ms | entropy_ms | assemble_ms |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    med = {}
    for (name, lib), rs in groups.items():
        ms = [x for r in rs for x in r["engine_ms"]]
        py = [x for r in rs for x in r["wall_ms"]]
        med[(name, lib)] = (statistics.median(ms), min(ms), max(ms))
        last = rs[-1]
        print(f"| {name} | {lib} | {last['outputs']} | {len(ms)} | {statistics.median(ms):.1f} | {min(ms):.1f} .. {max(ms):.1f} | "
              f"{statistics.median(py):.1f} | "
              f"{last['parsed'] or '-'} | {last['parse_run_ms']} | {last['scale_ms']} | {last['jpeg_ms']} | {last['entropy_ms']} | {last['assemble_ms']} |")
    if ("plain", "this") in med:
        c = med[("plain", "this")]
        print(f"\nRun-to-run spread of (c), engine time: {c[2] - c[1]:.1f} ms (median {c[0]:.1f}).\n")
        for s in ("03", "0123"):
            a, b = med.get(("multi" + s, "this")), med.get(("old" + s, "parent")) or med.get(("old" + s, "this"))
            if a and b:
                print(f"- [{', '.join(s)}]: (a) {a[0]:.1f} ms = {a[0] / c[0]:.2f} x (c); (b) {b[0]:.1f} ms = {b[0] / c[0]:.2f} x (c); "
                      f"(b) - (a) = {b[0] - a[0]:.1f} ms")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="mode", required=True)

    def common(p):
        p.add_argument("--n", type=int, default=1024)
        p.add_argument("--set", default="bench")
        p.add_argument("--threads", type=int, default=0)
        p.add_argument("--width", type=int, default=1920)
        p.add_argument("--height", type=int, default=1080)
        p.add_argument("--limit", type=int, default=240, help="seconds per GPU step")

    p = sub.add_parser("k3p")
    p.add_argument("dir")
    common(p)
    p = sub.add_parser("e2e")
    p.add_argument("dir")
    p.add_argument("--parent-lib", default=None, help="directory of an older build's libraries")
    p.add_argument("--passes", type=int, default=2)
    p.add_argument("--reps", type=int, default=3)
    common(p)
    p = sub.add_parser("k3p-run")
    common(p)
    p = sub.add_parser("case")
    p.add_argument("--case", choices=CASES, required=True)
    p.add_argument("--reps", type=int, default=3)
    common(p)
    for name, fn in (("summarise-k3p", summarise_k3p), ("summarise-e2e", summarise_e2e)):
        p = sub.add_parser(name)
        p.add_argument("dir")
        common(p)
    args = ap.parse_args()
    {"k3p": k3p, "e2e": e2e, "k3p-run": k3p_run, "case": case, "summarise-k3p": summarise_k3p,
     "summarise-e2e": summarise_e2e}[args.mode](args)


if __name__ == "__main__":
    main()
