"""Mint the committed HEVC test vectors and benchmark inputs (test infrastructure).

Source content: the reference's own fixture test/img/img01.h265 (tests/golden/),
decoded by the oracle, cropped / flipped / upsampled, plus seeded Gaussian
noise (SURVEY.md §8d recipe).  Encoded with tools/hevcgen (our HEVC intra
encoder; the container has no other HEVC encoder).  Every stream is checked
here: the oracle's pre-loop-filter decode must equal hevcgen's own
reconstruction bit-for-bit.

  python tools/make_streams.py bench   -> tests/golden/bench/hevc1080_XX.h265 (16 streams)
  python tools/make_streams.py parity  -> tests/golden/hevc/*.h265 + manifest.json
  python tools/make_streams.py 4k      -> tests/golden/bench4k/hevc2160_10b_XX.h265
  python tools/make_streams.py parity264 -> tests/golden/h264/*.h264 + manifest.json (tools/h264gen)
  python tools/make_streams.py wide264   -> tests/golden/h264wide/*.h264 (line buffer in global memory)
  python tools/make_streams.py tall264   -> tests/golden/h264tall/*.h264 (banded K1 / deblocking, 10-bit)
  python tools/make_streams.py bench264  -> tests/golden/bench264/avc1080_XX.h264 (16 streams, High 8x8)
  python tools/make_streams.py mixed     -> tests/golden/mixed/ (720p H.265/H.264, 4K H.264) for configs[4]
  python tools/make_streams.py f3        -> tests/golden/f3/ (decoder delay, non-IDR / CRA / BLA first pictures)
  python tools/make_streams.py malformed -> tests/golden/malformed/ (out-of-range SPS / slice header values)
  python tools/make_streams.py heavy     -> tests/golden/bench_heavy/hevc1080h_XX.h265 (16 streams, ~100-250 KB)
  python tools/make_streams.py heif      -> tests/golden/heif/ (tile pictures of HEIF grids, sets a-e, and H.264 tiles)
  python tools/make_streams.py colour    -> tests/golden/colour/ (VUI video_signal_type: matrix and range signalled, or not)
  python tools/make_streams.py k0levels  -> tests/golden/k0levels/ (designed levels up to the int16 range: K0's clips)
  python tools/make_streams.py aim       -> tests/golden/bench_aim/hevc1080a_XX.h265 (64 streams, QP 22-37, 110-220 KB)
"""
import glob
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_py as O  # noqa: E402

GEN = os.path.join(ROOT, "tools", "hevcgen", "hevcgen")
GEN264 = os.path.join(ROOT, "tools", "h264gen", "h264gen")


def build_gen():
    for gen in (GEN, GEN264):
        src = gen + ".c"
        if not os.path.exists(gen) or os.path.getmtime(gen) < os.path.getmtime(src):
            subprocess.check_call(["gcc", "-O2", "-o", gen, src, "-lm"])


def source_planes():
    y, u, v, _ = O.decode(open(os.path.join(ROOT, "tests/golden/img01.h265"), "rb").read(), 265)
    return y.astype(np.int32), u.astype(np.int32), v.astype(np.int32)


def make_content(planes, W, H, seed, sigma, bd, upsample=1):
    rng = np.random.default_rng(seed)
    y, u, v = planes
    if upsample > 1:
        y = np.repeat(np.repeat(y, upsample, 0), upsample, 1)
        u = np.repeat(np.repeat(u, upsample, 0), upsample, 1)
        v = np.repeat(np.repeat(v, upsample, 0), upsample, 1)
    Hs, Ws = y.shape
    x0 = int(rng.integers(0, (Ws - W) // 2 + 1)) * 2
    y0 = int(rng.integers(0, (Hs - H) // 2 + 1)) * 2
    out = []
    hf, vf = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
    for c, p in enumerate((y, u, v)):
        s = 1 if c == 0 else 2
        q = p[y0 // s:(y0 + H) // s, x0 // s:(x0 + W) // s].astype(np.float64)
        if hf:
            q = q[:, ::-1]
        if vf:
            q = q[::-1, :]
        scale = 1 << (bd - 8)
        q = q * scale
        if bd > 8:
            q = q + rng.integers(0, scale, q.shape)  # fill the low bits
        if sigma:
            q = q + rng.normal(0, sigma * scale, q.shape)
        out.append(np.clip(np.rint(q), 0, (1 << bd) - 1).astype(np.int32))
    return out


def encode(planes, W, H, bd, qp, seed, path, opts=(), codec=265):
    yuv = path + ".yuv"
    rec = path + ".rec"
    dt = np.uint8 if bd == 8 else np.dtype("<u2")
    with open(yuv, "wb") as f:
        for p in planes:
            f.write(p.astype(dt).tobytes())
    subprocess.check_call([GEN if codec == 265 else GEN264, yuv, str(W), str(H), str(bd), str(qp), str(seed), path, "--recon", rec] + list(opts))
    s = open(path, "rb").read()
    y, u, v, b = O.decode(s, codec, skip_loop_filter=True)
    r = np.fromfile(rec, dtype=dt).astype(np.int32)
    ys, cs = W * H, (W // 2) * (H // 2)
    ok = (np.array_equal(y, r[:ys].reshape(H, W)) and np.array_equal(u, r[ys:ys + cs].reshape(H // 2, W // 2))
          and np.array_equal(v, r[ys + cs:].reshape(H // 2, W // 2)))
    os.remove(yuv)
    os.remove(rec)
    if not ok:
        raise SystemExit(f"{path}: oracle decode != encoder reconstruction")
    return len(s)


def bench(n=16):
    out_dir = os.path.join(ROOT, "tests/golden/bench")
    os.makedirs(out_dir, exist_ok=True)
    planes = source_planes()
    qps = [22, 27, 32, 37]
    sigmas = [0, 2, 4]
    total = 0
    for i in range(n):
        qp, sigma = qps[i % 4], sigmas[(i // 4) % 3]
        content = make_content(planes, 1920, 1080, i, sigma, 8)
        path = os.path.join(out_dir, f"hevc1080_{i:02d}.h265")
        nb = encode(content, 1920, 1080, 8, qp, i, path)
        total += nb
        print(f"{path}: qp {qp} sigma {sigma} -> {nb} B", flush=True)
    print("total", total)


def heavy(n=16):
    """configs[1] on heavier content: ~100-250 KB per 1080p picture (SURVEY.md §8(d) aim);
    the host CABAC cost scales with it (the end-to-end bound)."""
    out_dir = os.path.join(ROOT, "tests/golden/bench_heavy")
    os.makedirs(out_dir, exist_ok=True)
    planes = source_planes()
    qps = [18, 20, 22, 24]
    sigmas = [0, 1, 2, 1]
    total = 0
    for i in range(n):
        qp, sigma = qps[i % 4], sigmas[(i // 4) % 4]
        content = make_content(planes, 1920, 1080, 400 + i, sigma, 8)
        path = os.path.join(out_dir, f"hevc1080h_{i:02d}.h265")
        nb = encode(content, 1920, 1080, 8, qp, 400 + i, path)
        total += nb
        print(f"{path}: qp {qp} sigma {sigma} -> {nb} B", flush=True)
    print("total", total, "mean", total // n)


def aim(n=64):
    """configs[1] exactly as SURVEY.md §8(d) specifies it: QP cycling {22, 27, 32, 37},
    seeded crops / flips of the fixture content plus Gaussian noise, 100-250 KB per 1080p picture.  The
    noise level is searched per stream (starting from a per-QP guess) until the picture lands in
    [110, 220] KB, so every QP contributes pictures of the aimed size.  64 distinct streams (seeds
    700..763), tiled x16 into the bench's 1024-picture batch: the bench's headline workload."""
    out_dir = os.path.join(ROOT, "tests/golden/bench_aim")
    os.makedirs(out_dir, exist_ok=True)
    planes = source_planes()
    qps = [22, 27, 32, 37]
    guess = {22: 2.0, 27: 4.0, 32: 7.5, 37: 11.0}
    total = 0
    rows = []
    for i in range(n):
        qp, seed = qps[i % 4], 700 + i
        path = os.path.join(out_dir, f"hevc1080a_{i:02d}.h265")
        lo, hi, sigma = 0.0, 24.0, guess[qp] + 0.5 * ((i // 4) % 3 - 1)
        for _ in range(8):
            content = make_content(planes, 1920, 1080, seed, sigma, 8)
            nb = encode(content, 1920, 1080, 8, qp, seed, path)
            if nb < 110_000:
                lo = sigma
            elif nb > 220_000:
                hi = sigma
            else:
                break
            sigma = (lo + hi) / 2 if hi < 24.0 else sigma * 1.25 + 0.5
        else:
            raise SystemExit(f"{path}: no noise level within 110-220 KB")
        total += nb
        rows.append({"file": os.path.basename(path), "qp": qp, "sigma": round(sigma, 3), "bytes": nb})
        print(f"{path}: qp {qp} sigma {sigma:.3f} -> {nb} B", flush=True)
    json.dump(rows, open(os.path.join(out_dir, "manifest.json"), "w"), indent=1)
    print("total", total, "mean", total // n)


def nosdh(n=2):
    """configs[1]-sized pictures with sign-data hiding off: the path img01.h265 (the reference
    fixture) pins, exercised at 1080p as well (bench streams use --sdh 1, hevcgen's default)."""
    out_dir = os.path.join(ROOT, "tests/golden/bench_nosdh")
    os.makedirs(out_dir, exist_ok=True)
    planes = source_planes()
    for i, (qp, sigma) in enumerate([(22, 2), (32, 0)][:n]):
        content = make_content(planes, 1920, 1080, 500 + i, sigma, 8)
        path = os.path.join(out_dir, f"hevc1080_nosdh_{i:02d}.h265")
        nb = encode(content, 1920, 1080, 8, qp, 500 + i, path, ["--sdh", "0"])
        print(f"{path}: qp {qp} sigma {sigma} -> {nb} B", flush=True)


def entropy():
    """High-entropy pictures for the JPEG payload emitter: 512x256 HEVC, QP 4, uniform
    noise in 32 rows (the top rows, or rows 96..127) and flat grey elsewhere, so the noisy 256-block
    tiles carry more than 32 JPEG bytes per block (K5d's global-memory path, kEmitWords) while the
    flat tiles beside them stay on the LDS path (tests/test_entropy_vectors.py checks both)."""
    out_dir = os.path.join(ROOT, "tests/golden/entropy")
    os.makedirs(out_dir, exist_ok=True)
    for f in glob.glob(os.path.join(out_dir, "*.h265")):
        os.remove(f)
    W, H = 512, 256
    rng = np.random.default_rng(7)
    for name, r0 in (("noise_top", 0), ("noise_mid", 96)):
        y = np.full((H, W), 128, np.uint8)
        u = np.full((H // 2, W // 2), 128, np.uint8)
        v = u.copy()
        y[r0:r0 + 32] = rng.integers(0, 256, (32, W))
        u[r0 // 2:r0 // 2 + 16] = rng.integers(0, 256, (16, W // 2))
        v[r0 // 2:r0 // 2 + 16] = rng.integers(0, 256, (16, W // 2))
        path = os.path.join(out_dir, f"{name}_512x256_q4.h265")
        nb = encode([y.astype(np.int32), u.astype(np.int32), v.astype(np.int32)], W, H, 8, 4, 7, path)
        print(f"{path}: {nb} B", flush=True)


PARITY = [
    # name, W, H, bd, qp, seed, sigma, options
    ("p01_416x240_q22", 416, 240, 8, 22, 11, 2, []),
    ("p02_416x240_q37_nosdh", 416, 240, 8, 37, 12, 0, ["--sdh", "0"]),
    ("p03_400x232_pcm_bypass_slices", 400, 232, 8, 30, 13, 3, ["--pcm", "1", "--bypass", "1", "--slices", "1"]),
    ("p04_416x240_10bit_ctb32_d2", 416, 240, 10, 27, 14, 2, ["--pcm", "1", "--ctb", "32", "--depth", "2"]),
    ("p05_256x144_ctb16_offsets", 256, 144, 8, 18, 15, 4, ["--ctb", "16", "--cbqp", "3", "--crqp", "-2", "--beta", "2", "--tc", "-1"]),
    ("p06_352x288_q12_noise", 352, 288, 8, 12, 16, 4, []),
    ("p07_336x200_q45", 336, 200, 8, 45, 17, 0, ["--beta", "-3", "--tc", "4"]),
    ("p08_320x180_10bit_q2", 320, 180, 10, 2, 18, 3, ["--depth", "0"]),
    ("p09_200x120_noqpd_notskip", 200, 120, 8, 24, 19, 2, ["--qpdelta", "0", "--tskip", "0", "--sao", "0"]),
    ("p10_480x272_slices2", 480, 272, 8, 31, 20, 1, ["--slices", "2", "--bypass", "1"]),
    ("p11_64x64_tiny", 64, 64, 8, 26, 21, 2, []),
    ("p12_72x40_odd_crop", 72, 40, 8, 26, 22, 2, ["--ctb", "16"]),
    ("p13_416x240_wpp", 416, 240, 8, 27, 23, 2, ["--wpp", "1"]),
    ("p14_480x272_wpp_slices_ctb32", 480, 272, 8, 30, 24, 2, ["--wpp", "1", "--slices", "2", "--ctb", "32"]),
    ("p15_48x200_wpp_narrow", 48, 200, 8, 26, 25, 2, ["--wpp", "1"]),
    ("p16_1280x720_wpp_ctb32", 1280, 720, 8, 24, 26, 3, ["--wpp", "1", "--ctb", "32"]),
    # black top third: PCM samples of 0 put emulation-prevention bytes inside WPP substreams
    ("p17_416x240_10bit_wpp_pcm_black", 416, 240, 10, 30, 28, 0, ["--wpp", "1", "--pcm", "1", "--ctb", "32"]),
    ("p18_416x240_tiles3x2_ctb32", 416, 240, 8, 28, 29, 2, ["--ctb", "32", "--tilecols", "3", "--tilerows", "2"]),
    ("p19_480x272_tiles2x2_wpp_nolf", 480, 272, 8, 30, 30, 2, ["--ctb", "32", "--tilecols", "2", "--tilerows", "2", "--wpp", "1", "--lftiles", "0"]),
    ("p20_80x96_tiles5x3_wpp_narrow", 80, 96, 8, 26, 31, 2, ["--ctb", "16", "--tilecols", "5", "--tilerows", "3", "--wpp", "1"]),
    # scaling lists (7.3.4 / 7.4.5): SPS defaults (Table 7-6), explicit SPS lists (DC, pred_matrix_id_delta
    # copies, defaults), explicit PPS lists over explicit / default SPS lists
    ("p21_416x240_sl_sps_default", 416, 240, 8, 25, 32, 2, ["--sl", "1"]),
    ("p22_416x240_sl_sps_explicit", 416, 240, 8, 22, 33, 3, ["--sl", "2", "--depth", "2"]),
    ("p23_480x272_sl_sps_pps_ctb32", 480, 272, 8, 30, 34, 2, ["--sl", "3", "--ctb", "32", "--bypass", "1"]),
    ("p24_352x288_10bit_sl_pps_over_default", 352, 288, 10, 20, 35, 2, ["--sl", "4", "--pcm", "1"]),
    # 9- and 12-bit 4:2:0 (FFmpeg yuv420p9 / yuv420p12; RExt profile), SAO offsets unscaled at 12 bits
    ("p26_416x240_9bit", 416, 240, 9, 27, 36, 2, ["--pcm", "1", "--bypass", "1"]),
    ("p27_416x240_12bit", 416, 240, 12, 24, 37, 2, ["--pcm", "1", "--depth", "2"]),
    # range extensions (--rext bits: 1 ts rotation, 2 ts contexts, 4 implicit RDPCM, 8 explicit RDPCM,
    # 32 intra smoothing off, 64 high-precision offsets, 128 persistent Rice adaptation)
    ("p28_416x240_12bit_rext_all", 416, 240, 12, 22, 38, 3,
     ["--rext", "167", "--maxts", "5", "--saoscale", "2,1", "--bypass", "1", "--vui", "1"]),
    ("p29_416x240_rext_ts_rdpcm_rice_wpp", 416, 240, 8, 26, 39, 2,
     ["--profile", "4", "--rext", "135", "--maxts", "4", "--bypass", "1", "--wpp", "1", "--ctb", "32"]),
    ("p30_352x288_10bit_rext_nosmooth_rice_slices", 352, 288, 10, 20, 40, 2,
     ["--profile", "4", "--rext", "160", "--slices", "1", "--depth", "2", "--maxts", "3"]),
    # Main profile with a VUI and a pps_range_extension the decoder must ignore (not RExt)
    ("p31_416x240_vui_ppsext_ignored", 416, 240, 8, 28, 41, 2, ["--vui", "1", "--ppsext", "1", "--maxts", "5"]),
    # RExt flags without effect on intra pictures, chroma QP offset list present but off in the slice
    ("p32_320x192_rext_noop_cqo_list", 320, 192, 8, 30, 42, 2,
     ["--profile", "4", "--rext", "75", "--cqo", "1", "--tilecols", "2"]),
    # VERDICT r05 #1 (round 6): what FFmpeg 4.3 decodes and round 5 rejected.  extended_precision_processing
    # and cabac_bypass_alignment are read and ignored ("not yet implemented"); at <= 9 bits extended
    # precision changes nothing else (Max(15, BitDepth + 6) = 15).  CU chroma QP offsets
    # (cu_chroma_qp_offset_flag / _idx per chroma QP offset group) enter the Cb / Cr dequantisation QP.
    # p33-p35 are round 5's malformed/m_hevc_rext_{extprec,bypass_align,cqo_slice} recipes.
    ("p33_160x96_rext_extprec", 160, 96, 8, 27, 82, 2, ["--rext", "16"]),
    ("p34_160x96_rext_bypass_align", 160, 96, 8, 27, 83, 2, ["--rext", "256"]),
    ("p35_160x96_rext_cqo_slice", 160, 96, 8, 27, 84, 2, ["--profile", "4", "--cqo", "2"]),
    ("p36_416x240_extprec_8bit_rice_bypass", 416, 240, 8, 22, 43, 3,
     ["--profile", "4", "--rext", "144", "--bypass", "1", "--pcm", "1"]),
    ("p37_416x240_cqo_list6_depth2", 416, 240, 8, 26, 44, 3,
     ["--profile", "4", "--cqo", "2", "--cqolist", "-12,12,5,-5,0,0,3,7,-6,-2,10,-9", "--cqodepth", "2",
      "--bypass", "1", "--cbqp", "2", "--crqp", "-1"]),
    ("p38_352x288_10bit_cqo_list3_wpp", 352, 288, 10, 24, 45, 2,
     ["--profile", "4", "--cqo", "2", "--cqolist", "-4,2,6,-3,1,1", "--cqodepth", "0", "--wpp", "1", "--ctb", "32"]),
    ("p39_320x192_9bit_extprec_cqo_tiles", 320, 192, 9, 20, 46, 3,
     ["--rext", "16", "--cqo", "2", "--cqolist", "3,-3,-5,5,2,2", "--cqodepth", "3", "--tilecols", "2", "--ctb", "32"]),
]


def parity():
    out_dir = os.path.join(ROOT, "tests/golden/hevc")
    os.makedirs(out_dir, exist_ok=True)
    planes = source_planes()
    manifest = []
    for name, W, H, bd, qp, seed, sigma, opts in PARITY:
        content = make_content(planes, W, H, seed, sigma, bd)
        if "black" in name:
            content[0][: H // 3] = 0
        path = os.path.join(out_dir, name + ".h265")
        nb = encode(content, W, H, bd, qp, seed, path, opts)
        manifest.append({"file": name + ".h265", "w": W, "h": H, "bit_depth": bd, "qp": qp, "options": opts})
        print(f"{path}: {nb} B", flush=True)
    json.dump(manifest, open(os.path.join(out_dir, "manifest.json"), "w"), indent=1)
    leftcrop()  # p25 (its own recipe) stays in the manifest


PARITY264 = [
    # name, W, H, bd, qp, seed, sigma, options   (h264gen)
    ("a01_416x240_q22_main", 416, 240, 8, 22, 31, 2, ["--t8x8", "0"]),
    ("a02_416x240_q30_high8x8", 416, 240, 8, 30, 32, 2, ["--t8x8", "1"]),
    ("a03_400x232_pcm_slices", 400, 232, 8, 28, 33, 3, ["--pcm", "1", "--slices", "3"]),
    ("a04_352x288_10bit_high10", 352, 288, 10, 27, 34, 2, ["--pcm", "1"]),
    ("a05_256x144_cqp_offsets", 256, 144, 8, 18, 35, 4, ["--cqp", "4", "--cqp2", "-3", "--alpha", "3", "--beta", "-2"]),
    ("a06_352x288_q12_noise", 352, 288, 8, 12, 36, 6, []),
    ("a07_336x200_q45", 336, 200, 8, 45, 37, 0, ["--alpha", "-4", "--beta", "5"]),
    ("a08_320x176_dbidc1", 320, 176, 8, 26, 38, 3, ["--dbidc", "1"]),
    ("a09_480x272_dbidc2_slices", 480, 272, 8, 33, 39, 2, ["--dbidc", "2", "--slices", "2"]),
    ("a10_200x120_noqpd", 200, 120, 8, 24, 40, 2, ["--qpdelta", "0"]),
    ("a11_64x64_tiny", 64, 64, 8, 26, 41, 2, []),
    ("a12_72x40_odd_crop", 72, 40, 8, 20, 42, 5, ["--pcm", "1"]),
    ("a13_320x180_10bit_q0", 320, 180, 10, 0, 43, 4, ["--t8x8", "0", "--cqp", "-5"]),
    # CAVLC (entropy_coding_mode_flag 0)
    ("a14_416x240_cavlc_main", 416, 240, 8, 26, 44, 2, ["--cavlc", "1", "--t8x8", "0"]),
    ("a15_352x288_cavlc_high8x8_pcm", 352, 288, 8, 20, 45, 4, ["--cavlc", "1", "--pcm", "1"]),
    ("a16_320x176_cavlc_10bit", 320, 176, 10, 12, 46, 6, ["--cavlc", "1"]),
    ("a17_256x144_cavlc_q0_noise", 256, 144, 8, 0, 47, 20, ["--cavlc", "1", "--t8x8", "1"]),
    ("a18_480x272_cavlc_slices_offsets", 480, 272, 8, 33, 48, 2,
     ["--cavlc", "1", "--slices", "2", "--cqp", "2", "--alpha", "1", "--beta", "-1"]),
    # scaling matrices (7.3.2.1.1.1): SPS lists (fall-back rule A), SPS + PPS lists (rule B),
    # PPS lists only (rule A in the PPS); useDefaultScalingMatrixFlag and early-ended lists
    ("a19_416x240_sm_sps_8x8", 416, 240, 8, 24, 49, 2, ["--sm", "1"]),
    ("a20_416x240_sm_sps_pps_8x8", 416, 240, 8, 30, 50, 3, ["--sm", "2", "--cqp", "2", "--cqp2", "-1"]),
    ("a21_352x288_sm_pps_cavlc", 352, 288, 8, 20, 51, 2, ["--sm", "3", "--cavlc", "1"]),
    ("a22_320x176_sm_sps_pps_10bit_4x4", 320, 176, 10, 16, 52, 3, ["--sm", "2", "--t8x8", "0"]),
    # interlace-capable SPS (frame_mbs_only_flag 0) coding a frame picture without MBAFF: height in
    # field MB rows, vertical crop in 4-row units, field_pic_flag in the slice header
    ("a23_416x232_ilsps_frame", 416, 232, 8, 27, 55, 2, ["--ilsps", "1", "--slices", "4"]),
    ("a24_336x180_ilsps_frame_cavlc", 336, 180, 8, 24, 56, 3, ["--ilsps", "1", "--cavlc", "1"]),
    # High 4:4:4 Predictive (profile_idc 244): lossless transform bypass (qpprime_y_zero_transform_bypass_flag,
    # QP'Y 0, residual DPCM for vertical / horizontal predictions) and 4:2:0 at 12 / 14 bits
    ("a25_176x144_lossless_cabac", 176, 144, 8, 0, 57, 6, ["--lossless", "1", "--pcm", "1"]),
    ("a26_192x112_lossless_cavlc_4x4", 192, 112, 8, 0, 58, 8, ["--lossless", "1", "--cavlc", "1", "--t8x8", "0"]),
    ("a27_208x128_lossless_14bit", 208, 128, 14, 0, 59, 5, ["--lossless", "1"]),
    ("a28_256x144_12bit_high444", 256, 144, 12, 22, 60, 4, ["--t8x8", "1", "--slices", "3"]),
    ("a29_192x112_14bit_cavlc_pcm", 192, 112, 14, 14, 61, 6, ["--cavlc", "1", "--pcm", "1"]),
    ("a30_160x96_lossless_10bit_slices", 160, 96, 10, 0, 62, 4, ["--lossless", "1", "--slices", "2"]),
    # MBAFF frames (frame_mbs_only_flag 0, mb_adaptive_frame_field_flag 1): macroblock pairs coded as
    # two frame or two field macroblocks (6.4.12.2 neighbours, field scans and contexts, 8.7 MBAFF
    # deblocking); a36 is a 1080i-sized frame
    ("a31_336x192_mbaff_cabac_8x8", 336, 192, 8, 24, 63, 6, ["--mbaff", "1", "--t8x8", "1", "--slices", "4"]),
    ("a32_320x160_mbaff_cavlc_4x4_pcm", 320, 160, 8, 22, 64, 5, ["--mbaff", "1", "--cavlc", "1", "--t8x8", "0", "--pcm", "1"]),
    ("a33_352x224_mbaff_10bit_dbidc2", 352, 224, 10, 27, 65, 4, ["--mbaff", "1", "--slices", "4", "--dbidc", "2"]),
    ("a34_256x128_mbaff_all_field", 256, 128, 8, 20, 70, 10, ["--mbaff", "1", "--fieldpct", "100", "--alpha", "3", "--beta", "2"]),
    ("a35_240x96_mbaff_cavlc_8x8_offsets", 240, 96, 8, 18, 71, 12, ["--mbaff", "1", "--cavlc", "1", "--cqp", "3", "--cqp2", "-2"]),
    ("a36_1920x1080_mbaff_1080i", 1920, 1080, 8, 26, 68, 3, ["--mbaff", "1", "--t8x8", "1"]),
    # PAFF field pairs (field_pic_flag 1): an IDR I field and a non-IDR I field of the other parity,
    # decoded as the frame FFmpeg outputs after the second field (the reference itself returns false
    # for a field picture: one packet, "Wait for second field"); --paff 2 = bottom field first
    ("a37_320x192_paff_cabac_8x8_slices", 320, 192, 8, 24, 72, 6, ["--paff", "1", "--t8x8", "1", "--slices", "2"]),
    ("a38_256x160_paff_botfirst_cavlc_dbidc2", 256, 160, 8, 22, 73, 5, ["--paff", "2", "--cavlc", "1", "--slices", "2", "--dbidc", "2"]),
    ("a39_192x128_paff_10bit_pcm_offsets", 192, 128, 10, 26, 74, 8, ["--paff", "1", "--pcm", "1", "--cqp", "2", "--alpha", "2", "--beta", "-1"]),
    ("a40_1920x1080_paff_1080i", 1920, 1080, 8, 26, 75, 3, ["--paff", "1", "--t8x8", "1"]),
    # 4:0:0 (High profile monochrome): no chroma syntax; FFmpeg outputs yuv420p with
    # chroma 1 << (BitDepth - 1); crop units 1 x (2 - frame_mbs_only)
    ("a41_400x232_mono_cabac_8x8_pcm", 400, 232, 8, 26, 76, 3, ["--mono", "1", "--pcm", "1", "--slices", "3"]),
    ("a42_336x192_mono_cavlc_10bit", 336, 192, 10, 24, 77, 4, ["--mono", "1", "--cavlc", "1", "--pcm", "1"]),
    ("a43_320x160_mono_mbaff_cavlc", 320, 160, 8, 22, 78, 5, ["--mono", "1", "--mbaff", "1", "--cavlc", "1", "--t8x8", "0"]),
    ("a44_256x144_mono_paff_12bit", 256, 144, 12, 20, 79, 4, ["--mono", "1", "--paff", "1", "--t8x8", "1"]),
    ("a45_208x128_mono_lossless", 208, 128, 8, 0, 80, 6, ["--mono", "1", "--lossless", "1", "--pcm", "1"]),
]


def parity264():
    out_dir = os.path.join(ROOT, "tests/golden/h264")
    os.makedirs(out_dir, exist_ok=True)
    planes = source_planes()
    manifest = []
    for name, W, H, bd, qp, seed, sigma, opts in PARITY264:
        content = make_content(planes, W, H, seed, sigma, bd)
        path = os.path.join(out_dir, name + ".h264")
        nb = encode(content, W, H, bd, qp, seed, path, opts, codec=264)
        manifest.append({"file": name + ".h264", "w": W, "h": H, "bit_depth": bd, "qp": qp, "options": opts})
        print(f"{path}: {nb} B", flush=True)
    json.dump(manifest, open(os.path.join(out_dir, "manifest.json"), "w"), indent=1)


def bench264(n=16):
    """Config 3: 1080p H.264 High (8x8 transform) I-frames; streams 7 and 15
    are CAVLC (2/16 = 12.5 %, SURVEY.md §8d asks for a ~10 % CAVLC mix)."""
    out_dir = os.path.join(ROOT, "tests/golden/bench264")
    os.makedirs(out_dir, exist_ok=True)
    planes = source_planes()
    qps = [22, 27, 32, 37]
    sigmas = [0, 2, 4]
    total = 0
    for i in range(n):
        qp, sigma = qps[i % 4], sigmas[(i // 4) % 3]
        content = make_content(planes, 1920, 1080, 200 + i, sigma, 8)
        path = os.path.join(out_dir, f"avc1080_{i:02d}.h264")
        opts = ["--t8x8", "1"] + (["--cavlc", "1"] if i % 8 == 7 else [])
        nb = encode(content, 1920, 1080, 8, qp, 200 + i, path, opts, codec=264)
        total += nb
        print(f"{path}: qp {qp} sigma {sigma} -> {nb} B", flush=True)
    print("total", total)


def heavy264(n=16):
    """configs[2] on heavier content: ~100-250 KB per 1080p picture (SURVEY.md §8(d) aim), the
    value_aim set of the avc1080 bench line; streams 3 and 11 are CAVLC (2/16, the §8(d) mix)."""
    out_dir = os.path.join(ROOT, "tests/golden/bench264_heavy")
    os.makedirs(out_dir, exist_ok=True)
    planes = source_planes()
    qps = [18, 20, 22, 24]
    sigmas = [0, 1, 0, 1]
    total = 0
    for i in range(n):
        qp, sigma = qps[i % 4], sigmas[(i // 4) % 4]
        content = make_content(planes, 1920, 1080, 600 + i, sigma, 8)
        path = os.path.join(out_dir, f"avc1080h_{i:02d}.h264")
        opts = ["--t8x8", "1"] + (["--cavlc", "1"] if i % 8 == 3 else [])
        nb = encode(content, 1920, 1080, 8, qp, 600 + i, path, opts, codec=264)
        total += nb
        print(f"{path}: qp {qp} sigma {sigma} -> {nb} B", flush=True)
    print("total", total, "mean", total // n)


def mixed():
    """configs[4] ingredients: 720p H.265 + H.264, 4K H.264 (1080p and 4K H.265
    come from the bench / bench4k sets)."""
    out_dir = os.path.join(ROOT, "tests/golden/mixed")
    os.makedirs(out_dir, exist_ok=True)
    planes = source_planes()
    for i, qp in enumerate([22, 27, 32, 37]):
        content = make_content(planes, 1280, 720, 300 + i, 2, 8)
        nb = encode(content, 1280, 720, 8, qp, 300 + i, os.path.join(out_dir, f"hevc720_{i:02d}.h265"))
        print(f"hevc720_{i:02d}: {nb} B", flush=True)
        opts = ["--t8x8", "1"] + (["--cavlc", "1"] if i == 3 else [])
        nb = encode(content, 1280, 720, 8, qp, 310 + i, os.path.join(out_dir, f"avc720_{i:02d}.h264"), opts, codec=264)
        print(f"avc720_{i:02d}: {nb} B", flush=True)
    for i, qp in enumerate([27, 32]):
        content = make_content(planes, 3840, 2160, 320 + i, 2, 8, upsample=2)
        nb = encode(content, 3840, 2160, 8, qp, 320 + i, os.path.join(out_dir, f"avc2160_{i:02d}.h264"), ["--t8x8", "1"],
                    codec=264)
        print(f"avc2160_{i:02d}: {nb} B", flush=True)


F3 = [
    # decoder-delay streams (the reference returns false without output for
    # these, /root/reference/src/Decoder.cpp:342-360: avcodec_receive_frame gives EAGAIN after
    # one packet; we transcode picture 0) and leading non-IDR / CRA / BLA pictures.
    # name, codec, W, H, qp, seed, options
    ("f3_avc_delay2", 264, 352, 288, 26, 60, ["--delay", "2"]),
    ("f3_avc_nonidr_first", 264, 416, 240, 28, 61, ["--nonidr", "1", "--slices", "5"]),
    ("f3_avc_nonidr_delay1_cavlc", 264, 320, 176, 24, 62, ["--nonidr", "1", "--delay", "1", "--cavlc", "1"]),
    ("f3_hevc_delay2", 265, 352, 288, 27, 63, ["--delay", "2"]),
    ("f3_hevc_cra_first", 265, 416, 240, 27, 64, ["--nut", "21", "--slices", "2"]),
    ("f3_hevc_bla_first_delay1", 265, 320, 184, 30, 65, ["--nut", "16", "--delay", "1", "--ctb", "32"]),
    ("f3_hevc_cra_wpp", 265, 480, 272, 25, 66, ["--nut", "21", "--wpp", "1"]),
]


def f3():
    out_dir = os.path.join(ROOT, "tests/golden/f3")
    os.makedirs(out_dir, exist_ok=True)
    planes = source_planes()
    manifest = []
    for name, codec, W, H, qp, seed, opts in F3:
        content = make_content(planes, W, H, seed, 2, 8)
        ext = ".h265" if codec == 265 else ".h264"
        path = os.path.join(out_dir, name + ext)
        nb = encode(content, W, H, 8, qp, seed, path, opts, codec=codec)
        delay = "--delay" in opts
        manifest.append({"file": name + ext, "codec": codec, "w": W, "h": H, "options": opts,
                         "reference_returns": False if delay else None,
                         "note": "decoder delay: reference silently returns false (EAGAIN, no flush)" if delay
                         else "leading intra picture without IDR: reference result unpinned (FFmpeg recovery logic)"})
        print(f"{path}: {nb} B", flush=True)
    json.dump(manifest, open(os.path.join(out_dir, "manifest.json"), "w"), indent=1)


MALFORMED = [
    # parameter-set values outside their ranges.  FFmpeg 4.3 (the reference path)
    # rejects an H.264 SPS whose cropping leaves no picture (h264_ps.c "crop values invalid",
    # goto fail) but ignores such an HEVC conformance window (hevc_ps.c "Invalid cropping
    # offsets ... Displaying the whole video surface"); "ok" = a JPEG of the whole coded
    # picture, "fail" = no JPEG.
    # name, codec, W, H, options, expect
    ("m_avc_crop_overflow", 264, 400, 232, ["--crop", "0,300,0,0"], "fail"),
    ("m_avc_crop_huge", 264, 400, 232, ["--crop", "2147483647,0,5,4"], "fail"),
    ("m_avc_firstmb_oob", 264, 128, 96, ["--firstmb", "100000"], "fail"),
    ("m_hevc_conf_overflow", 265, 396, 228, ["--conf", "0,250,0,0"], "ok"),
    ("m_hevc_conf_huge", 265, 396, 228, ["--conf", "4294967294,0,0,4294967294"], "ok"),
    ("m_hevc_width_not_mincb", 265, 128, 96, ["--wdelta", "4"], "fail"),
    # FFmpeg 4.3 h264_ps.c fails the SPS on max_num_reorder_frames > 16 and on an HRD
    # with cpb_cnt_minus1 > 31; the same VUI fields in range decode
    ("m_avc_vui_reorder17", 264, 160, 96, ["--vuireorder", "17"], "fail"),
    ("m_avc_vui_cpb33", 264, 160, 96, ["--vuicpb", "32", "--vuireorder", "0"], "fail"),
    ("m_avc_vui_cpb32_ok", 264, 160, 96, ["--vuicpb", "31", "--vuireorder", "0"], "ok"),
    # FFmpeg 4.3 has no 11- / 13-bit H.264 output format (h264_slice.c "Unsupported bit depth")
    ("m_avc_bitdepth11", 264, 160, 96, ["@bd", "11"], "fail"),
    # a PAFF field without the other parity's field: FFmpeg outputs no frame for it
    ("m_avc_paff_one_field", 264, 160, 96, ["--paff", "1", "--onefield", "1"], "fail"),
    # FFmpeg has no 11-bit HEVC pixel format.  The three "moved" slots (round 5's extended-precision,
    # bypass-alignment and CU chroma QP offset streams, which FFmpeg 4.3 decodes) became the parity
    # vectors p33-p35; the slots stay so the later entries keep their seeds
    ("m_hevc_rext_extprec", 265, 160, 96, [], "moved"),
    ("m_hevc_rext_bypass_align", 265, 160, 96, [], "moved"),
    ("m_hevc_rext_cqo_slice", 265, 160, 96, [], "moved"),
    ("m_hevc_bitdepth11", 265, 160, 96, ["@bd", "11"], "fail:bit depth"),
    # left crops as FFmpeg 4.3 applies them (decode.c apply_cropping -> av_frame_apply_cropping, which
    # lowers crop_left to keep the planes 32-byte aligned: 8-bit 4:2:0 to a multiple of 64, 16-bit to
    # a multiple of 32; AVERROR_BUG, no frame, when a plane's alignment exceeds the crop's)
    ("m_avc_crop_left8", 264, 400, 232, ["--crop", "4,0,0,4"], "ok"),
    ("m_hevc_conf_left16", 265, 400, 232, ["--conf", "8,0,0,0"], "ok"),
    ("m_hevc_conf_left48_10bit", 265, 400, 240, ["@bd", "10", "--conf", "24,0,4,0"], "ok"),
    ("m_avc_mono_crop_left1", 264, 160, 96, ["--mono", "1", "--crop", "1,0,0,0"], "ok"),
    ("m_avc_mono_crop_left3_10bit", 264, 160, 96, ["@bd", "10", "--mono", "1", "--crop", "3,0,0,0"], "fail:AVERROR_BUG"),
]


def malformed():
    out_dir = os.path.join(ROOT, "tests/golden/malformed")
    os.makedirs(out_dir, exist_ok=True)
    planes = source_planes()
    manifest = []
    for k, (name, codec, W, H, opts, expect) in enumerate(MALFORMED):
        if expect == "moved":
            continue
        bd = int(opts[1]) if opts[:1] == ["@bd"] else 8  # "@bd N": the stream's bit depth
        gopts = opts[2:] if opts[:1] == ["@bd"] else opts
        content = make_content(planes, W, H, 70 + k, 2, bd)
        ext = ".h265" if codec == 265 else ".h264"
        path = os.path.join(out_dir, name + ext)
        yuv = path + ".yuv"
        with open(yuv, "wb") as f:
            for p in content:
                f.write(p.astype(np.uint8 if bd == 8 else np.dtype("<u2")).tobytes())
        subprocess.check_call([GEN if codec == 265 else GEN264, yuv, str(W), str(H), str(bd), "27", str(70 + k), path]
                              + gopts)
        os.remove(yuv)
        e = {"file": name + ext, "codec": codec, "options": opts, "expect": expect.split(":")[0]}
        if ":" in expect:
            e["message"] = expect.split(":", 1)[1]  # substring of the picture's own error message
        manifest.append(e)
        print(f"{path}: {os.path.getsize(path)} B, expect {expect}", flush=True)
    json.dump(manifest, open(os.path.join(out_dir, "manifest.json"), "w"), indent=1)


def leftcrop():
    """an HEVC picture whose conformance window starts 64 luma samples from the
    left and 16 from the top, with an output of 336x224 (16-aligned), so K3 SAO sums the JPEG rate
    control's MB variances (h2j_sao_folds_variance).  The cropped-away left columns are noise and
    the kept picture is smooth, so summing them would move qscale.  Written into tests/golden/hevc
    (the parity suite: planes, JPEG, mixed batches).  The oracle's cropped decode must equal the
    encoder's reconstruction inside the window."""
    out_dir = os.path.join(ROOT, "tests/golden/hevc")
    planes = source_planes()
    W, H, cl, ct = 400, 240, 64, 16
    content = make_content(planes, W, H, 36, 0, 8)
    rng = np.random.default_rng(36)
    content[0][:, :cl] = rng.integers(0, 256, (H, cl))
    for c in (1, 2):
        content[c][:, :cl // 2] = rng.integers(0, 256, (H // 2, cl // 2))
    name = "p25_400x240_conf_left64_top16"
    path = os.path.join(out_dir, name + ".h265")
    yuv, rec = path + ".yuv", path + ".rec"
    with open(yuv, "wb") as f:
        for p in content:
            f.write(p.astype(np.uint8).tobytes())
    subprocess.check_call([GEN, yuv, str(W), str(H), "8", "26", "36", path, "--recon", rec,
                           "--conf", f"{cl // 2},0,{ct // 2},0"])
    y, u, v, _ = O.decode(open(path, "rb").read(), 265, skip_loop_filter=True)
    r = np.fromfile(rec, dtype=np.uint8).astype(np.int32)
    ys, cs = W * H, (W // 2) * (H // 2)
    ry = r[:ys].reshape(H, W)[ct:, cl:]
    ru = r[ys:ys + cs].reshape(H // 2, W // 2)[ct // 2:, cl // 2:]
    rv = r[ys + cs:].reshape(H // 2, W // 2)[ct // 2:, cl // 2:]
    os.remove(yuv)
    os.remove(rec)
    if not (np.array_equal(y, ry) and np.array_equal(u, ru) and np.array_equal(v, rv)):
        raise SystemExit(f"{path}: oracle decode != encoder reconstruction (window)")
    man_path = os.path.join(out_dir, "manifest.json")
    manifest = [m for m in json.load(open(man_path)) if m["file"] != name + ".h265"]
    manifest.append({"file": name + ".h265", "w": W, "h": H, "bit_depth": 8, "qp": 26,
                     "options": ["--conf", f"{cl // 2},0,{ct // 2},0"], "output": [W - cl, H - ct]})
    json.dump(manifest, open(man_path, "w"), indent=1)
    print(f"{path}: {os.path.getsize(path)} B, output {y.shape[1]}x{y.shape[0]}", flush=True)


WIDE264 = [
    # wide pictures.  r05: the 8-bit deblocking kernel holds an LDS line buffer for any legal
    # width (8192 = 512 MBs, the parser's limit) and the 16-bit one up to ~6.6K columns, so w03
    # (8192 wide, 10-bit) is the vector on the global line-buffer path (h2j_k2_deblock264p, GLine);
    # w01 / w02 keep the widest LDS line buffers
    ("w01_8192x48_wide", 8192, 48, 8, 28, 53, 3, ["--slices", "2"]),
    ("w02_6144x32_wide_10bit", 6144, 32, 10, 24, 54, 2, ["--t8x8", "0"]),
    ("w03_8192x32_wide_10bit", 8192, 32, 10, 26, 55, 2, ["--slices", "2"]),
]


def wide264():
    out_dir = os.path.join(ROOT, "tests/golden/h264wide")
    os.makedirs(out_dir, exist_ok=True)
    planes = source_planes()
    manifest = []
    for name, W, H, bd, qp, seed, sigma, opts in WIDE264:
        up = -(-W // planes[0].shape[1])
        content = make_content(planes, W, H, seed, sigma, bd, upsample=up)
        path = os.path.join(out_dir, name + ".h264")
        nb = encode(content, W, H, bd, qp, seed, path, opts, codec=264)
        manifest.append({"file": name + ".h264", "w": W, "h": H, "bit_depth": bd, "qp": qp, "options": opts})
        print(f"{path}: {nb} B", flush=True)
    json.dump(manifest, open(os.path.join(out_dir, "manifest.json"), "w"), indent=1)


TALL264 = [
    # pictures taller than 68 MB rows run H.264 K1 in 8-row bands (k1map8) and the
    # deblocking in 16-row bands; a 10-bit one covers h264_rows<uint16_t> band hand-offs, and a second
    # banded picture of another height shares a batch with it
    ("t01_256x1152_tall_10bit", 256, 1152, 10, 26, 90, 3, ["--t8x8", "1", "--slices", "5"]),
    ("t02_192x1408_tall_cavlc", 192, 1408, 8, 24, 91, 3, ["--cavlc", "1", "--pcm", "1"]),
]


def tall264():
    out_dir = os.path.join(ROOT, "tests/golden/h264tall")
    os.makedirs(out_dir, exist_ok=True)
    planes = source_planes()
    manifest = []
    for name, W, H, bd, qp, seed, sigma, opts in TALL264:
        up = -(-H // planes[0].shape[0])
        content = make_content(planes, W, H, seed, sigma, bd, upsample=up)
        path = os.path.join(out_dir, name + ".h264")
        nb = encode(content, W, H, bd, qp, seed, path, opts, codec=264)
        manifest.append({"file": name + ".h264", "w": W, "h": H, "bit_depth": bd, "qp": qp, "options": opts})
        print(f"{path}: {nb} B", flush=True)
    json.dump(manifest, open(os.path.join(out_dir, "manifest.json"), "w"), indent=1)


def fourk(n=4):
    out_dir = os.path.join(ROOT, "tests/golden/bench4k")
    os.makedirs(out_dir, exist_ok=True)
    planes = source_planes()
    for i in range(n):
        qp = [22, 27, 32, 37][i % 4]
        content = make_content(planes, 3840, 2160, 100 + i, [0, 2][i % 2], 10, upsample=2)
        path = os.path.join(out_dir, f"hevc2160_10b_{i:02d}.h265")
        nb = encode(content, 3840, 2160, 10, qp, 100 + i, path)
        print(f"{path}: qp {qp} -> {nb} B", flush=True)


HEIF_SETS = [
    # HEIF grid tile sets (tests/heif_mux.py wraps them at test time): name, tile w, h, CTB, tiles, bit depth, QP,
    # options.  The smallest shapes at which a canvas of tiles can still go wrong; QP >= 32 with SAO on, so that
    # deblocking and SAO act at every tile border; one option set per set, so that all tiles share one SPS and PPS
    ("a", 64, 64, 16, 4, 8, 34, []),                  # 2 x 2 -> 120 x 100
    ("b", 64, 64, 64, 6, 8, 36, []),                  # 3 x 2 -> 192 x 128: one CTB per tile
    ("c", 64, 32, 32, 3, 8, 33, []),                  # 1 x 3 and 3 x 1
    ("d", 128, 128, 32, 4, 10, 32, ["--slices", "2"]),  # 2 x 2, Main10, two slices per tile picture
    ("e", 256, 256, 64, 6, 8, 35, []),                # 3 x 2 -> 700 x 500: several K1 pool rows, cropped last row / column
]


def _ps_nals(stream):
    """the SPS and PPS NAL units of an HEVC Annex-B stream"""
    parts = stream.replace(b"\x00\x00\x00\x01", b"\x00\x00\x01").split(b"\x00\x00\x01")
    return [p for p in parts if p and ((p[0] >> 1) & 63) in (33, 34)]


def heif():
    """tests/golden/heif/: tile pictures for HEIF grids (named .hevc / .avc: they are tiles, not the pictures the
    stream suites walk).  Each set is one crop of the source content cut into equal tiles, every tile encoded on its
    own with the set's options; the SPS and PPS bytes must come out identical across the tiles of a set."""
    out_dir = os.path.join(ROOT, "tests/golden/heif")
    os.makedirs(out_dir, exist_ok=True)
    planes = source_planes()
    manifest = []
    for name, tw, th, ctb, n, bd, qp, opts in HEIF_SETS:
        cols = 3 if n in (3, 6) else 2
        rows = n // cols
        canvas = make_content(planes, cols * tw, rows * th, 700 + ord(name), 6, bd)  # (noise: residuals at QP >= 32)
        ps = None
        for t in range(n):
            ty, tx = divmod(t, cols)
            tile = [canvas[0][ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw]] + [
                p[ty * th // 2:(ty + 1) * th // 2, tx * tw // 2:(tx + 1) * tw // 2] for p in canvas[1:]]
            path = os.path.join(out_dir, f"{name}_{t}.hevc")
            nb = encode(tile, tw, th, bd, qp, 7000 + 16 * ord(name) + t, path, ["--ctb", str(ctb), "--sao", "1"] + opts)
            got = _ps_nals(open(path, "rb").read())
            if ps is not None and got != ps:
                raise SystemExit(f"{path}: SPS / PPS differ from tile 0's (seed-dependent parameter sets)")
            ps = got
            print(f"{path}: {nb} B", flush=True)
            if name == "a" and t == 1:
                # the same tile once more with a PPS-level option (pps_cb_qp_offset): its SPS must be the set's and
                # only its PPS differ -- the vector for "tiles carry different PPS"
                path = os.path.join(out_dir, "a_1_pps.hevc")
                encode(tile, tw, th, bd, qp, 7000 + 16 * ord(name) + t, path, ["--ctb", str(ctb), "--sao", "1", "--cbqp", "2"] + opts)
                odd = _ps_nals(open(path, "rb").read())
                if [p for p in odd if (p[0] >> 1) & 63 == 33] != [p for p in ps if (p[0] >> 1) & 63 == 33] or odd == ps:
                    raise SystemExit(f"{path}: --cbqp must change the PPS and leave the SPS alone")
        manifest.append({"set": name, "tile_w": tw, "tile_h": th, "ctb": ctb, "tiles": n, "bit_depth": bd, "qp": qp, "options": opts})
    canvas = make_content(planes, 128, 128, 790, 1, 8)
    for t in range(4):  # H.264 tiles: a grid of them is rejected
        ty, tx = divmod(t, 2)
        tile = [canvas[0][ty * 64:(ty + 1) * 64, tx * 64:(tx + 1) * 64]] + [p[ty * 32:(ty + 1) * 32, tx * 32:(tx + 1) * 32] for p in canvas[1:]]
        path = os.path.join(out_dir, f"h264_{t}.avc")
        print(f"{path}: {encode(tile, 64, 64, 8, 32, 7900 + t, path, [], codec=264)} B", flush=True)
    manifest.append({"set": "h264", "tile_w": 64, "tile_h": 64, "tiles": 4, "bit_depth": 8, "qp": 32, "options": []})
    json.dump(manifest, open(os.path.join(out_dir, "manifest.json"), "w"), indent=1)


# (file, codec, W, H, bit depth, qp, --colour P,T,M,F or None: no VUI): what colour="auto" has to read
COLOUR_SETS = [
    ("c709_limited.hevc", 265, 96, 64, 8, 30, (1, 1, 1, 0)),
    ("c2020_limited_10b.hevc", 265, 64, 48, 10, 30, (9, 16, 9, 0)),
    ("c709_full.avc", 264, 64, 64, 8, 28, (1, 1, 1, 1)),
    ("cnodesc_full.hevc", 265, 48, 32, 8, 32, (2, 2, -1, 1)),  # a full-range flag and no colour description
    ("cnovui.avc", 264, 48, 48, 8, 30, None),
    ("cmc8_ycgco.hevc", 265, 32, 32, 8, 32, (1, 1, 8, 0)),    # a matrix the library does not convert
]


def colour():
    """tests/golden/colour/: small pictures whose SPS signals a colour matrix and range, or does not (named .hevc /
    .avc: the stream suites do not walk them).  manifest.json states what each signals -- primaries, transfer, matrix,
    full range; 2 / 2 / 2 / 0 where absent -- so the tests never ask the parser under test."""
    out_dir = os.path.join(ROOT, "tests/golden/colour")
    os.makedirs(out_dir, exist_ok=True)
    planes = source_planes()
    manifest = []
    for i, (name, codec, w, h, bd, qp, col) in enumerate(COLOUR_SETS):
        content = make_content(planes, w, h, 900 + i, 3, bd)
        path = os.path.join(out_dir, name)
        opts = [] if col is None else ["--colour", ",".join(str(x) for x in col)]
        nb = encode(content, w, h, bd, qp, 9000 + i, path, opts, codec=codec)
        sig = (2, 2, 2, 0) if col is None else ((col[0], col[1], col[2]) if col[2] >= 0 else (2, 2, 2)) + (col[3],)
        manifest.append({"file": name, "codec": codec, "w": w, "h": h, "bit_depth": bd, "qp": qp, "vui": col is not None,
                         "primaries": sig[0], "transfer": sig[1], "matrix": sig[2], "full_range": sig[3]})
        print(f"{path}: {nb} B", flush=True)
    json.dump(manifest, open(os.path.join(out_dir, "manifest.json"), "w"), indent=1)

# (name, tier, bit depth, qp, seed, options): tests/golden/k0levels/.  The QPs put Qp'Y near 22 (tier 1) / 28 (tier 2)
# at every bit depth, so that the dequantisation scale of a 32x32 block is above 1 and a level of 32767 clips
K0LEVELS = [
    ("a08", 1, 8, 22, 1, []),
    ("a10", 1, 10, 10, 2, []),
    ("a12", 1, 12, -2, 3, []),
    ("a08_sl", 1, 8, 24, 4, ["--sl", "2"]),
    ("a12_ts32", 1, 12, 0, 5, ["--profile", "4", "--maxts", "5"]),
    ("b08", 2, 8, 28, 6, []),
    ("b10", 2, 10, 16, 17, []),
    ("b12", 2, 12, 4, 8, []),
    ("b10_sl", 2, 10, 14, 9, ["--sl", "3"]),
]


def k0levels_content(bd, seed):
    """128 x 128, sixteen 32 x 32 CTBs: piecewise-constant luma whose pieces are 32 (twelve CTBs), 16 (two), 8 and 4
    (one each) samples wide, so that the encoder's variance rule makes coding blocks, and with them transform blocks,
    of every size; a little noise gives the blocks that are not injected a residual of their own"""
    rng = np.random.default_rng(seed)
    sc = 1 << (bd - 8)
    kinds = [32, 32, 16, 32, 32, 8, 32, 32, 32, 32, 4, 32, 16, 32, 32, 32]
    y = np.zeros((128, 128))
    for i, b in enumerate(kinds):
        ty, tx = divmod(i, 4)
        piece = 128 + rng.integers(-40, 41, (32 // b, 32 // b)) if b < 32 else np.full((1, 1), 128 + rng.integers(-8, 9))
        y[ty * 32:ty * 32 + 32, tx * 32:tx * 32 + 32] = np.kron(piece, np.ones((b, b)))
    y = y * sc + rng.normal(0, 0.5 * sc, y.shape)
    c = [np.full((64, 64), 128.0 * sc) + rng.normal(0, 0.5 * sc, (64, 64)) for _ in range(2)]
    return [np.clip(np.rint(p), 0, (1 << bd) - 1).astype(np.int32) for p in [y] + c]


def k0levels():
    """tests/golden/k0levels/: pictures whose transform blocks carry hevcgen's --inject patterns (levels up to 32767 and
    -32768), tier 1 large but inside every clip of 8.6.2-8.6.4, tier 2 past them; three of four blocks are injected.
    manifest.json keeps each vector's options and its census by tests/k0_ref.py, which tests/test_k0_levels.py
    recomputes and holds against the conditions the vectors are there for."""
    import tempfile

    import k0_ref as K
    out_dir = os.path.join(ROOT, "tests/golden/k0levels")
    os.makedirs(out_dir, exist_ok=True)
    manifest = []
    with tempfile.TemporaryDirectory() as tmp:
        exe = K.build_dumper(os.path.join(tmp, "tu_dump"))
        for name, tier, bd, qp, seed, opts in K0LEVELS:
            path = os.path.join(out_dir, f"{name}.h265")
            opts = ["--ctb", "32", "--depth", "0", "--inject", f"{tier},3,4"] + opts  # (depth 0: a 32 x 32 CU is one TB)
            nb = encode(k0levels_content(bd, 1100 + seed), 128, 128, bd, qp, 1100 + seed, path, opts)
            K.dump(exe, [(path, os.path.join(tmp, "d.bin"))])
            manifest.append({"file": f"{name}.h265", "tier": tier, "w": 128, "h": 128, "bit_depth": bd, "qp": qp,
                             "seed": 1100 + seed, "options": opts, "census": K.census(os.path.join(tmp, "d.bin"))})
            print(f"{path}: {nb} B", flush=True)
    json.dump(manifest, open(os.path.join(out_dir, "manifest.json"), "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    build_gen()
    what = sys.argv[1] if len(sys.argv) > 1 else "bench"
    {"bench": bench, "parity": parity, "4k": fourk, "parity264": parity264, "bench264": bench264,
     "mixed": mixed, "f3": f3, "heavy": heavy, "malformed": malformed, "nosdh": nosdh, "entropy": entropy,
     "wide264": wide264, "leftcrop": leftcrop, "heavy264": heavy264, "tall264": tall264, "aim": aim, "heif": heif,
     "colour": colour, "k0levels": k0levels}[what]()
