"""HEVC scaling and transformation (H.265 8.6.2-8.6.4) of transform-block records, restated in numpy int64.

The input is what the host parser hands K0 (tools/parse_bench/tu_dump.cpp: h2j_tu records, coefficient entries,
scaling factors, header); the output is each block's residual and a census of the three places where the
arithmetic has to clip, which the committed streams must never reach unnoticed (tests/test_k0_levels.py).

Written from the specification, not from the kernel:
  * 8.6.3: d = Clip3(-32768, 32767, (level * m * levelScale[qP % 6] << (qP / 6)) + (1 << (bdShift - 1)) >> bdShift),
    bdShift = BitDepth + Log2(nTbS) - 5, m = 16 or the ScalingFactor (16 too for transform-skip blocks above 4x4);
  * 8.6.4.2: transMatrix (the 32-point matrix; smaller ones are its rows 0, 32/N, 2*32/N, ... cut to N columns),
    the 4x4 DST-VII matrix, first stage down the columns (+64 >> 7, Clip3 to 16 bits), second stage along the
    rows, then bdShift = 20 - BitDepth;
  * transform skip: rotation of 4x4 blocks (range extensions), r = d << tsShift, tsShift = 5 + Log2(nTbS), then the
    same bdShift; cu_transquant_bypass: r = level; implicit RDPCM for both (modes 10 and 26).
Where the specification leaves a value wider than 16 bits the project follows FFmpeg's int16 coefficient buffer
(DESIGN.md section 5): the second stage is clipped to int16 like the first, a transform-skip left shift and the RDPCM
sums wrap.  Each of those is counted, so a stream with a zero census is pinned by the specification alone.

Blocks of one size are processed together (arrays [blocks, N, N]); all sums are int64.
"""
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_dumper(exe):
    """tools/parse_bench/tu_dump over the host parser, built as tests/test_parse_digests.py builds parse_bench"""
    host = os.path.join(ROOT, "h264-h265-to-jpeg_amd", "csrc", "host")
    clang = os.path.join(os.environ.get("ROCM", "/opt/rocm"), "llvm", "bin", "clang++")
    cxx, tune = (clang, ["-mtune=znver5"]) if os.path.exists(clang) else (shutil.which("g++"), [])
    srcs = [os.path.join(ROOT, "tools", "parse_bench", "tu_dump.cpp")] + [
        os.path.join(host, f) for f in ("bitstream.cpp", "cabac_tables.cpp", "hevc_parser.cpp", "h264_parser.cpp")]
    subprocess.check_call([cxx, "-std=c++11", "-O3", "-march=x86-64-v3", "-pthread"] + tune +
                          ["-I", os.path.join(ROOT, "include"), "-I", host] + srcs + ["-o", exe])
    return exe


def dump(exe, pairs):
    """pairs of (stream path, dump path) through one tu_dump process"""
    subprocess.check_call([exe] + [p for pair in pairs for p in pair])


LEVEL_SCALE = (40, 45, 51, 57, 64, 72)
TU_CBF, TU_TSKIP, TU_BYPASS, TU_PCM, TU_DST = 1, 2, 4, 8, 128
REXT_RDPCM, REXT_TS_ROT = 1, 2
SL_OFF = {2: 0, 3: 48, 4: 240, 5: 1008}  # FrameJob::sl: [size][component][y * N + x]

TU_DTYPE = np.dtype([("x", "<u2"), ("y", "<u2"), ("log2n", "u1"), ("c", "u1"), ("mode", "u1"), ("flags", "u1"),
                     ("qp", "i1"), ("qpy", "i1"), ("ncoef", "<u2"), ("coef", "<u4")])
HEAD = ("codec", "width", "height", "bit_depth", "bit_depth_c", "log2ctb", "scaling_list", "rext", "ntu", "ncoef", "nsl")


def _dct32():
    """transMatrix of 8.6.4.2: entry [m][n] is +-c[k], k the angle (2n + 1) * m folded into the first quadrant"""
    c = [64, 90, 90, 90, 89, 88, 87, 85, 83, 82, 80, 78, 75, 73, 70, 67, 64, 61, 57, 54, 50, 46, 43, 38, 36, 31, 25,
         22, 18, 13, 9, 4, 0]
    m = np.zeros((32, 32), np.int64)
    for r in range(32):
        for n in range(32):
            a = ((2 * n + 1) * r) % 128  # angle in units of pi / 64
            if a > 64:
                a = 128 - a              # cos(2 pi - t) = cos t
            m[r, n] = -c[64 - a] if a > 32 else c[a]  # cos(pi - t) = -cos t
    return m


DCT32 = _dct32()
DST4 = np.array([[29, 55, 74, 84], [74, 74, 0, -74], [84, -29, -74, 55], [55, -84, 74, -29]], np.int64)


def matrix(n, dst=False):
    """M[j][i]: coefficient j's contribution to output sample i"""
    return DST4 if dst else DCT32[::32 // n, :n]


def l1_max(n, dst=False):
    """largest L1 norm of a column of the matrix: bounds |sum_j M[j][i] * in[j]| / max |in|"""
    return int(np.abs(matrix(n, dst)).sum(axis=0).max())


def load(path):
    """a tu_dump file -> (header dict, TU records, coefficient entries uint32, scaling factors uint8)"""
    raw = open(path, "rb").read()
    assert raw[:4] == b"K0TU", path
    head = dict(zip(HEAD, np.frombuffer(raw, "<i4", len(HEAD), 4).tolist()))
    o = 4 + 4 * len(HEAD)
    tus = np.frombuffer(raw, TU_DTYPE, head["ntu"], o)
    o += 16 * head["ntu"]
    coefs = np.frombuffer(raw, "<u4", head["ncoef"], o)
    o += 4 * head["ncoef"]
    sl = np.frombuffer(raw, "u1", head["nsl"], o)
    assert o + head["nsl"] == len(raw), path
    return head, tus, coefs, sl


EVENTS = ("deq_pos", "deq_neg", "col_pos", "col_neg", "row_pos", "row_neg", "wrap")
MAXIMA = ("max_level", "max_deq", "max_col", "max_row")


def _rdpcm(r, vertical):
    """8.6.8 accumulation, in int16 as FFmpeg's coefficient buffer -> (residual, sums outside int16 per block)"""
    axis = 1 if vertical else 2
    s = np.cumsum(r, axis=axis)
    wraps = ((s < -32768) | (s > 32767)).sum(axis=(1, 2))
    return ((s + 32768) % 65536) - 32768, wraps


def blocks(head, tus, coefs, sl, log2n, select=None):
    """All residual-carrying (cbf, not PCM) records of size 1 << log2n, optionally only indices in `select`.
    -> dict: idx (record indices), res [B, N, N] int64 residuals, per-block event counts (EVENTS) and maxima (MAXIMA),
    each an int64 array [B]"""
    n = 1 << log2n
    fl = tus["flags"]
    idx = np.flatnonzero((tus["log2n"] == log2n) & ((fl & TU_CBF) != 0) & ((fl & TU_PCM) == 0) & (tus["ncoef"] > 0))
    if select is not None:
        idx = np.intersect1d(idx, np.asarray(select))
    B = len(idx)
    out = {"idx": idx, "res": np.zeros((B, n, n), np.int64)}
    for k in EVENTS + MAXIMA:
        out[k] = np.zeros(B, np.int64)
    if B == 0:
        return out
    t = tus[idx]
    # levels [B, N, N] from the entry lists
    cnt = t["ncoef"].astype(np.int64)
    blk = np.repeat(np.arange(B), cnt)
    ent = coefs[np.repeat(t["coef"].astype(np.int64), cnt) + (np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt))]
    pos = (ent >> 16).astype(np.int64)
    lvl = (ent & 0xFFFF).astype(np.uint16).view(np.int16).astype(np.int64)
    assert pos.max() < n * n
    level = np.zeros((B, n * n), np.int64)
    level[blk, pos] = lvl
    level = level.reshape(B, n, n)
    out["max_level"] = np.abs(level).max(axis=(1, 2))
    c = t["c"].astype(np.int64)
    bd = np.where(c > 0, head["bit_depth_c"], head["bit_depth"]).astype(np.int64)
    flags = t["flags"]
    bypass, tskip = (flags & TU_BYPASS) != 0, ((flags & TU_TSKIP) != 0) & ((flags & TU_BYPASS) == 0)
    dst = ((flags & TU_DST) != 0) & (log2n == 2)
    # 8.6.3 scaling
    m = np.full((B, n, n), 16, np.int64)
    if head["scaling_list"]:
        tab = sl[SL_OFF[log2n]:SL_OFF[log2n] + (1 if log2n == 5 else 3) * n * n].astype(np.int64).reshape(-1, n, n)
        use = ~(tskip & (n > 4))
        m[use] = tab[c[use] if log2n < 5 else np.zeros(int(use.sum()), np.int64)]
    qp = t["qp"].astype(np.int64)
    assert (qp >= 0).all()
    scale = np.array(LEVEL_SCALE, np.int64)[qp % 6] << (qp // 6)
    bd_shift = bd + log2n - 5
    v = (level * m * scale[:, None, None] + (1 << (bd_shift - 1))[:, None, None]) >> bd_shift[:, None, None]
    v[bypass] = 0
    out["deq_pos"], out["deq_neg"] = (v > 32767).sum(axis=(1, 2)), (v < -32768).sum(axis=(1, 2))
    out["max_deq"] = np.abs(v).max(axis=(1, 2))
    d = np.clip(v, -32768, 32767)
    res = np.zeros((B, n, n), np.int64)
    # cu_transquant_bypass
    res[bypass] = level[bypass]
    # transform skip
    if tskip.any():
        x = d[tskip]
        if (head["rext"] & REXT_TS_ROT) and n == 4:
            x = x[:, ::-1, ::-1]
        ts_shift, bs = 5 + log2n, (20 - bd[tskip])[:, None, None]
        r = ((x << ts_shift) + (1 << (bs - 1))) >> bs
        out["wrap"][tskip] = ((r < -32768) | (r > 32767)).sum(axis=(1, 2))
        res[tskip] = ((r + 32768) % 65536) - 32768
    if head["rext"] & REXT_RDPCM:
        for vertical in (True, False):
            sel = (bypass | tskip) & (t["mode"] == (26 if vertical else 10))
            if sel.any():
                res[sel], w = _rdpcm(res[sel], vertical)
                out["wrap"][sel] += w
    # 8.6.4.2 two-stage inverse transform
    for use_dst in (False, True):
        sel = ~bypass & ~tskip & (dst == use_dst)
        if not sel.any():
            continue
        M = matrix(n, use_dst)
        e = np.einsum("jy,bjx->byx", M, d[sel])          # first stage: down the columns
        g = (e + 64) >> 7
        out["col_pos"][sel], out["col_neg"][sel] = (g > 32767).sum(axis=(1, 2)), (g < -32768).sum(axis=(1, 2))
        out["max_col"][sel] = np.abs(g).max(axis=(1, 2))
        g = np.clip(g, -32768, 32767)
        bs = (20 - bd[sel])[:, None, None]
        r = (np.einsum("jx,byj->byx", M, g) + (1 << (bs - 1))) >> bs   # second stage: along the rows
        out["row_pos"][sel], out["row_neg"][sel] = (r > 32767).sum(axis=(1, 2)), (r < -32768).sum(axis=(1, 2))
        out["max_row"][sel] = np.abs(r).max(axis=(1, 2))
        res[sel] = np.clip(r, -32768, 32767)
    out["res"] = res
    out["c"], out["dst"], out["tskip"], out["bypass"], out["bd"] = c, dst, tskip, bypass, bd
    return out


def residual(head, tus, coefs, sl, i):
    """one record: (residual [N, N], {event: count}, {maximum: value})"""
    b = blocks(head, tus, coefs, sl, int(tus[i]["log2n"]), select=[i])
    assert len(b["idx"]) == 1, "record carries no residual"
    return b["res"][0], {k: int(b[k][0]) for k in EVENTS}, {k: int(b[k][0]) for k in MAXIMA}


CELLS = ("luma4dst", "luma4dct", "luma8", "luma16", "luma32", "chroma4", "chroma8", "chroma16")


def cell_names(b, log2n):
    """the census cell of each block of a blocks() result"""
    n = 1 << log2n
    if not len(b["idx"]):
        return np.array([], dtype=str)
    # (4x4 luma blocks that skip the transform carry no DST flag: they count with the intra 4x4 luma blocks)
    nodct = b["dst"] | b["tskip"] | b["bypass"]
    return np.array([("chroma%d" % n) if cc else ("luma4dst" if dd else "luma4dct") if n == 4 else "luma%d" % n
                     for cc, dd in zip(b["c"], nodct)])


def census(path):
    """{cell: {"tbs": blocks with residual, "transformed": blocks through the two-stage transform,
    events: blocks with at least one, maxima: largest}} of one tu_dump file (HEVC pictures only)"""
    head, tus, coefs, sl = load(path)
    assert head["codec"] == 265
    out = {}
    for log2n in (2, 3, 4, 5):
        b = blocks(head, tus, coefs, sl, log2n)
        names = cell_names(b, log2n)
        for cell in np.unique(names):
            s = names == cell
            rec = {"tbs": int(s.sum()), "transformed": int((s & ~b["tskip"] & ~b["bypass"]).sum())}
            for k in EVENTS:
                rec[k] = int((b[k][s] > 0).sum())
            for k in MAXIMA:
                rec[k] = int(b[k][s].max())
            # largest in-range first-stage output: what "large but unclipped" means for the column pass
            ok = s & (b["col_pos"] + b["col_neg"] + b["deq_pos"] + b["deq_neg"] == 0)
            rec["max_col_unclipped"] = int(b["max_col"][ok].max()) if ok.any() else 0
            out[str(cell)] = rec
    return out
