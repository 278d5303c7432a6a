// K3c: RGB output (DESIGN.md "RGB output (K3c)").  A rendition's final 8-bit planes -- what its JPEG source view
// shows K4 -- converted to 8-bit RGB, out of place: 4:2:0 planes -> w x h pixels, tightly packed, at
// h2j_rgb.dst_base + dst_off.  For the 8-bit planes Y (h x w) and Cb, Cr (h/2 x w/2), w and h even:
//   cx = x >> 1,  nx = clamp(cx + ((x & 1) ? 1 : -1), 0, w/2 - 1);   cy, ny likewise with y, h/2
//   C16(x, y) = 9 C[cy][cx] + 3 C[cy][nx] + 3 C[ny][cx] + C[ny][nx]          (0 .. 4080)
//   db = Cb16 - 2048,  dr = Cr16 - 2048
//   R = clip(((Y << 20) + 91881 dr + (1 << 19)) >> 20, 0, 255)
//   G = clip(((Y << 20) - 22554 db - 46802 dr + (1 << 19)) >> 20, 0, 255)
//   B = clip(((Y << 20) + 116130 db + (1 << 19)) >> 20, 0, 255)              (arithmetic shifts)
// JFIF's matrix in 16.16 on chroma kept at 16 x precision: one rounding, |sum| < 2^30, int32 throughout.  A source
// above 8 bits goes through K4's conversion first (min((v + (1 << (bd - 9))) >> (bd - 8), 255)), as in K3u.
//
// A workgroup is 64 lanes of 4 adjacent pixels x 4 lane rows.  Lane row j makes the output rows 2 j - 1 and 2 j
// (j = 0 .. h / 2: row -1 and row h do not exist): both take their chroma from the chroma rows j - 1 and j
// (clamped) -- the one its own, the other its vertical neighbour -- so a lane reads one chroma row pair and
// forms the horizontal sums 3 C[cx] + C[nx] of each once; row 2 j - 1 is 3 Ha + Hb, row 2 j is Ha + 3 Hb.
// Source rows, two forms:
//   wide  (h2j_rgb.wide: the 8-bit planes K3s / K3r / K3p / K3u wrote -- 16-byte row groups, no crop): one aligned
//         dword of Y a row; of each chroma row the lane's four samples 2 xd - 1 .. 2 xd + 2 (clamped to the plane's
//         w / 2 samples: the row padding is not what the clamp wants) lie in one or two dwords, both loaded.
//   plain (an unscaled frame, a window at any origin, an oriented source; uint8_t or uint16_t): clamped single
//         samples through the conversion.
// Nothing outside the source plane's samples (wide: its rows' whole dwords) is read.
// Stores: the pixels are tightly packed, so nothing lies behind a row to spill into: a lane stores exactly its
// pixels -- 4, or 2 at the end of a row with w % 4 == 2.  w % 4 == 0: rows start on dwords (3 w and w are
// multiples of 4; the output starts 256-byte aligned): three dwords a row interleaved, one a plane planar.
// w % 4 == 2: odd rows start 2 bytes off a dword: 16-bit stores (six a row interleaved, two a plane planar).
#include <hip/hip_runtime.h>

#include <cstdio>

#include "grid.h"
#include "h2j_gpu.h"

#define DEVI __host__ __device__ __forceinline__  // (host too: the lane code can be run and checked on a CPU)

namespace {

DEVI int k3c_to8(int v, int bd) {  // K4's 8-bit conversion (jpeg_sample)
    if (bd > 8) {
        v = (v + (1 << (bd - 9))) >> (bd - 8);
        v = v > 255 ? 255 : v;
    }
    return v;
}

// clip(v >> 20, 0, 255) of a 12.20 value, clamped before the shift: the same number (the shift floors, so it is
// monotone).  Why not clip(v >> 20): with hipcc of ROCm 7.2.0 (clang 22.0.0git roc-7.2.0) that form compiled to
// v_ashr_pk_u8_i32 whose result the plain classes ORed into the pixel dwords (v_or3_b32) unmasked, and on an MI355X
// bytes 2 and 3 of two of every three dwords then came out wrong, while the wide class, whose results went through
// v_perm_b32, was right.  Observed once, not reduced to a stand-alone reproducer: to see whether a later compiler
// still needs this form, write clip(v >> 20) back and run tests/test_gpu_rgb.py (its unscaled cases fail if so)
DEVI uint32_t k3c_clip20(int v) {
    v = v < 0 ? 0 : (v > (256 << 20) - 1 ? (256 << 20) - 1 : v);
    return static_cast<uint32_t>(v) >> 20;
}

// one 16-bit store (the W % 4 == 2 class).  A relaxed atomic store of wavefront scope is a plain global_store_short
// that hipcc may not merge with its neighbour: two plain 16-bit stores it merges into one dword store, which is
// misaligned on odd rows
DEVI void k3c_store16(uint8_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    __hip_atomic_store(reinterpret_cast<uint16_t*>(p), static_cast<uint16_t>(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
#else
    *reinterpret_cast<uint16_t*>(p) = static_cast<uint16_t>(v);
#endif
}

// luma row y (0 .. h - 1) of the lane: s[o] = Y(4 xd + o, y); wide: the row's dword (bytes past w: row padding,
// their pixels are not stored); plain: x clamped to the plane
template <typename Pel, bool Wide>
DEVI void k3c_luma(const Pel* __restrict__ P, int st, int w, int bd, int xd, int y, int (&s)[4]) {
    if constexpr (Wide) {
        const uint32_t c = reinterpret_cast<const uint32_t*>(P + static_cast<size_t>(y) * st)[xd];
        s[0] = c & 255;
        s[1] = (c >> 8) & 255;
        s[2] = (c >> 16) & 255;
        s[3] = c >> 24;
    } else {
#pragma unroll
        for (int o = 0; o < 4; o++) {
            const int x = min(4 * xd + o, w - 1);
            s[o] = k3c_to8(static_cast<int>(P[static_cast<size_t>(y) * st + x]), bd);
        }
    }
}

// chroma row r (0 .. ch - 1) of the lane: hs[o] = 3 C[cx] + C[nx] of pixel 4 xd + o, from the samples
// 2 xd - 1 .. 2 xd + 2 clamped to 0 .. cw - 1
template <typename Pel, bool Wide>
DEVI void k3c_chroma(const Pel* __restrict__ P, int st, int cw, int bd, int xd, int r, int (&hs)[4]) {
    int c[4];
    int idx[4];
#pragma unroll
    for (int k = 0; k < 4; k++) idx[k] = min(max(2 * xd - 1 + k, 0), cw - 1);
    if constexpr (Wide) {
        // the four indices are consecutive or repeat: they lie in the dword of the first or in that of the last
        const uint32_t* R = reinterpret_cast<const uint32_t*>(P + static_cast<size_t>(r) * st);
        const int d0 = idx[0] >> 2;
        const uint32_t lo = R[d0], hi = R[idx[3] >> 2];
#pragma unroll
        for (int k = 0; k < 4; k++) c[k] = static_cast<int>((((idx[k] >> 2) == d0 ? lo : hi) >> (8 * (idx[k] & 3))) & 255u);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) c[k] = k3c_to8(static_cast<int>(P[static_cast<size_t>(r) * st + idx[k]]), bd);
    }
    // pixels 4 xd + 0 .. 3: cx = 2 xd, 2 xd, 2 xd + 1, 2 xd + 1 (c[1], c[1], c[2], c[2]); nx = cx - 1, cx + 1, ...
    hs[0] = 3 * c[1] + c[0];
    hs[1] = 3 * c[1] + c[2];
    hs[2] = 3 * c[2] + c[1];
    hs[3] = 3 * c[2] + c[3];
}

// one output row of the lane: n pixels (4 or 2) from their luma and the 16 x chroma, stored at row y
template <bool Planar, bool Al4>
DEVI void k3c_store(uint8_t* __restrict__ O, int w, int h, int xd, int y, int n, const int (&Y)[4], const int (&cb16)[4],
                    const int (&cr16)[4]) {
    uint32_t px[4];  // R | G << 8 | B << 16
#pragma unroll
    for (int o = 0; o < 4; o++) {
        const int yy = (Y[o] << 20) + (1 << 19), db = cb16[o] - 2048, dr = cr16[o] - 2048;
        const uint32_t r = k3c_clip20(yy + 91881 * dr);
        const uint32_t g = k3c_clip20(yy - 22554 * db - 46802 * dr);
        const uint32_t b = k3c_clip20(yy + 116130 * db);
        px[o] = r | (g << 8) | (b << 16);
    }
    if constexpr (Planar) {
        const size_t plane = static_cast<size_t>(w) * h;
        uint8_t* row = O + static_cast<size_t>(y) * w + 4 * xd;
#pragma unroll
        for (int p = 0; p < 3; p++) {
            const uint32_t lo = ((px[0] >> (8 * p)) & 255u) | (((px[1] >> (8 * p)) & 255u) << 8);
            const uint32_t hi = ((px[2] >> (8 * p)) & 255u) | (((px[3] >> (8 * p)) & 255u) << 8);
            if constexpr (Al4) {
                *reinterpret_cast<uint32_t*>(row + p * plane) = lo | (hi << 16);
            } else {
                k3c_store16(row + p * plane, lo);
                if (n == 4) k3c_store16(row + p * plane + 2, hi);
            }
        }
    } else {
        uint8_t* row = O + static_cast<size_t>(y) * 3 * w + 12 * xd;
        // 12 bytes: R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
        const uint32_t d0 = px[0] | (px[1] << 24);
        const uint32_t d1 = (px[1] >> 8) | (px[2] << 16);
        const uint32_t d2 = (px[2] >> 16) | (px[3] << 8);
        if constexpr (Al4) {
            uint32_t* q = reinterpret_cast<uint32_t*>(row);
            q[0] = d0;
            q[1] = d1;
            q[2] = d2;
        } else {
            k3c_store16(row, d0);
            k3c_store16(row + 2, d0 >> 16);
            k3c_store16(row + 4, d1);
            if (n == 4) {
                k3c_store16(row + 6, d1 >> 16);
                k3c_store16(row + 8, d2);
                k3c_store16(row + 10, d2 >> 16);
            }
        }
    }
}

template <typename Pel, bool Wide, bool Planar, bool Al4>
DEVI void k3c_lane(uint8_t* __restrict__ arena, const h2j_rgb& rc, int xd, int j) {
    const int w = rc.w, h = rc.h, cw = w >> 1, ch = h >> 1;
    const Pel* S = reinterpret_cast<const Pel*>(arena + rc.src);
    const Pel* PY = S + rc.src_off[0] + static_cast<size_t>(rc.crop_y) * rc.src_stride[0] + rc.crop_x;
    const Pel* PU = S + rc.src_off[1] + static_cast<size_t>(rc.crop_y >> 1) * rc.src_stride[1] + (rc.crop_x >> 1);
    const Pel* PV = S + rc.src_off[2] + static_cast<size_t>(rc.crop_y >> 1) * rc.src_stride[2] + (rc.crop_x >> 1);
    // (h2j_rgb.dst_base is 0, the arena, until outputs in caller-owned memory come: the host will then pass that base
    // in the arena's place -- selecting it here made every store a flat one)
    uint8_t* O = arena + rc.dst_off;
    const int ra = max(j - 1, 0), rb = min(j, ch - 1);  // the chroma row pair
    int ua[4], ub[4], va[4], vb[4];
    k3c_chroma<Pel, Wide>(PU, rc.src_stride[1], cw, rc.bit_depth_c, xd, ra, ua);
    k3c_chroma<Pel, Wide>(PU, rc.src_stride[1], cw, rc.bit_depth_c, xd, rb, ub);
    k3c_chroma<Pel, Wide>(PV, rc.src_stride[2], cw, rc.bit_depth_c, xd, ra, va);
    k3c_chroma<Pel, Wide>(PV, rc.src_stride[2], cw, rc.bit_depth_c, xd, rb, vb);
    const int n = min(4, w - 4 * xd);  // w is even: 4 or 2
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int y = 2 * j - 1 + k;  // k = 0: the odd row above (its chroma row is ra), k = 1: the even row (rb)
        if (y < 0 || y >= h) continue;
        int Y[4], cb[4], cr[4];
        k3c_luma<Pel, Wide>(PY, rc.src_stride[0], w, rc.bit_depth, xd, y, Y);
#pragma unroll
        for (int o = 0; o < 4; o++) {
            cb[o] = k ? ua[o] + 3 * ub[o] : 3 * ua[o] + ub[o];
            cr[o] = k ? va[o] + 3 * vb[o] : 3 * va[o] + vb[o];
        }
        k3c_store<Planar, Al4>(O, w, h, xd, y, n, Y, cb, cr);
    }
}

template <typename Pel, bool Wide>
__global__ void __launch_bounds__(256) h2j_k3c_rgb(uint8_t* __restrict__ arena, const h2j_rgb* __restrict__ rmap) {
    // neighbouring tiles share their chroma halo rows and columns: the XCD-aware order (grid.h), as K3u
    const GridPos gp = xcd_grid_pos();
    const h2j_rgb& rc = rmap[gp.y];
    if ((rc.bit_depth > 8) != (sizeof(Pel) == 2) || (rc.wide != 0) != Wide) return;
    const int dw = (rc.w + 3) >> 2, tx = (dw + 63) >> 6, rows = (rc.h >> 1) + 1;
    const int t = gp.x;
    if (t >= tx * ((rows + 3) >> 2)) return;
    const int xd = (t % tx) * 64 + static_cast<int>(threadIdx.x & 63);
    const int j = (t / tx) * 4 + static_cast<int>(threadIdx.x >> 6);
    if (xd >= dw || j >= rows) return;
    // the layout and the row alignment are the output's: uniform over the workgroup
    const bool planar = rc.layout == 2, al4 = (rc.w & 3) == 0;
    if (planar) {
        if (al4) k3c_lane<Pel, Wide, true, true>(arena, rc, xd, j);
        else k3c_lane<Pel, Wide, true, false>(arena, rc, xd, j);
    } else {
        if (al4) k3c_lane<Pel, Wide, false, true>(arena, rc, xd, j);
        else k3c_lane<Pel, Wide, false, false>(arena, rc, xd, j);
    }
}

}  // namespace

namespace h2jgpu {  // defined in h2j_kernels.hip: one error slot for the whole C ABI
extern thread_local char g_err[256];
int check(hipError_t e, const char* what);
}  // namespace h2jgpu
using h2jgpu::check;
using h2jgpu::g_err;

extern "C" int h2j_gpu_rgb(const h2j_gpu_batch* b, const h2j_rgb* map, const int32_t* first, const int32_t* count,
                           const int32_t* tiles, void* stream) {
    if (!b || b->nframes <= 0) return 0;
    if (!map || !first || !count || !tiles) {
        snprintf(g_err, sizeof(g_err), "h2j_gpu_rgb: no map");
        return -1;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    // one launch per source class present: grid = the class's largest output x its outputs
    for (int cls = 0; cls < H2J_RGB_CLASSES; cls++) {
        if (count[cls] <= 0 || tiles[cls] <= 0) continue;
        const dim3 grid(static_cast<unsigned>(tiles[cls]), static_cast<unsigned>(count[cls]));
        const h2j_rgb* m = map + first[cls];
        switch (cls) {
        case 0: hipLaunchKernelGGL((h2j_k3c_rgb<uint8_t, true>), grid, dim3(256), 0, s, b->arena, m); break;
        case 1: hipLaunchKernelGGL((h2j_k3c_rgb<uint8_t, false>), grid, dim3(256), 0, s, b->arena, m); break;
        default: hipLaunchKernelGGL((h2j_k3c_rgb<uint16_t, false>), grid, dim3(256), 0, s, b->arena, m); break;
        }
        if (int rc = check(hipGetLastError(), "h2j_k3c_rgb")) return rc;
    }
    return 0;
}
