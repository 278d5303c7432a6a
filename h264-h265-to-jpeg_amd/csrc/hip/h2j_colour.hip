// K3v: colour (DESIGN.md "Colour (K3v)").  A rendition's 8-bit planes in the source's matrix (BT.601, BT.709, BT.2020
// non-constant luminance) and range (limited, full) -> 8-bit planes in JFIF's (BT.601, full range), out of place: the
// planes the rendition's view would otherwise be before finishing -> planes of their own (h2j_colour.dst), which K3u,
// K3b, K3c and K4 / K5 then read through the view.  With the record's constants k = oy, LY, LB, LR, CB, CR, RB, RR
// (include/h2j.h "Colour"), for the 8-bit planes Y (h x w) and Cb, Cr (h/2 x w/2), w and h even:
//   Cb16(x, y), Cr16(x, y): K3c's 9-3-3-1 chroma at luma position (x, y), 16 x precision (h2j_rgb.hip)
//   Y'(x, y)  = clip((LY (Y - oy) + LB (Cb16 - 2048) + LR (Cr16 - 2048) + (1 << 19)) >> 20, 0, 255)
//   Cb'(i, j) = clip((CB (Cb - 128) + CR (Cr - 128) + (128 << 16) + (1 << 15)) >> 16, 0, 255)
//   Cr'(i, j) = clip((RB (Cb - 128) + RR (Cr - 128) + (128 << 16) + (1 << 15)) >> 16, 0, 255)
// (arithmetic shifts; one rounding a sample; |sum| < 2^30: int32 throughout).  A source above 8 bits goes through K4's
// conversion first (min((v + (1 << (bd - 9))) >> (bd - 8), 255)), as in K3u.
//
// Two work classes (h2j_colour.matrix), each in K3u's three source classes:
//   matrix      a workgroup is 64 lanes of 8 adjacent luma samples x 4 lane rows.  Lane row j makes the luma rows
//               2 j - 1 and 2 j (j = 0 .. h / 2: row -1 and row h do not exist), which share the chroma rows j - 1 and j
//               (clamped), as in K3c: the horizontal sums 3 C[cx] + C[nx] of each are formed once; row 2 j - 1 is
//               3 Ha + Hb, row 2 j is Ha + 3 Hb.  The same lane converts the 4 samples of chroma row j (j < h / 2) of
//               both planes from the samples it holds.  Every store is a whole dword inside the destination's 16-byte
//               row groups: two a luma row, one a chroma row.
//   range only  LB = LR = CR = RB = 0: every plane is a map of its own samples.  Per plane, a workgroup is 64 dwords of
//               4 samples x 4 lane rows of H2J_K3V_ROWS rows: one load and one store a dword on a wide source.
// Source rows, two forms:
//   wide  (h2j_colour.wide: the 8-bit planes K3s / K3r / K3p wrote -- 16-byte row groups, no crop): aligned dword loads;
//         the matrix class takes the lane's chroma samples 4 xd - 1 .. 4 xd + 4 (clamped to the plane's w / 2 samples:
//         the row padding is not what the clamp wants) from the dwords xd - 1, xd, xd + 1 that hold them.
//   plain (an unscaled frame, a window at any origin, an oriented source; uint8_t or uint16_t): clamped single
//         samples through the conversion.
// All clamps are index clamps: nothing outside the source planes' rows (wide: their whole dwords) is read.  The last
// dwords of a destination row may run into its padding, never past it.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "grid.h"
#include "h2j_gpu.h"

#define DEVI __host__ __device__ __forceinline__  // (host too: the lane code can be run and checked on a CPU)

namespace {

DEVI int k3v_to8(int v, int bd) {  // K4's 8-bit conversion (jpeg_sample)
    if (bd > 8) {
        v = (v + (1 << (bd - 9))) >> (bd - 8);
        v = v > 255 ? 255 : v;
    }
    return v;
}

// clip(v >> S, 0, 255), clamped before the shift: the same number (the shift floors, so it is monotone), and the form
// K3c needs with this compiler (h2j_rgb.hip k3c_clip20, DESIGN.md "An observation about the compiler")
template <int S>
DEVI uint32_t k3v_clip(int v) {
    v = v < 0 ? 0 : (v > (256 << S) - 1 ? (256 << S) - 1 : v);
    return static_cast<uint32_t>(v) >> S;
}

// the single-sample accessor of the plain classes (K3u's): sample (x, y) of a w x h plane, both clamped, converted
template <typename Pel>
DEVI int k3v_at(const Pel* __restrict__ P, int st, int w, int h, int bd, int x, int y) {
    x = x < 0 ? 0 : (x > w - 1 ? w - 1 : x);
    y = y < 0 ? 0 : (y > h - 1 ? h - 1 : y);
    return k3v_to8(static_cast<int>(P[static_cast<size_t>(y) * st + x]), bd);
}

// chroma row r (0 .. ch - 1) of a matrix lane: c[k] = C[clamp(4 xd - 1 + k, 0, cw - 1)], k = 0 .. 5
template <typename Pel, bool Wide>
DEVI void k3v_chroma_row(const Pel* __restrict__ P, int st, int cw, int ch, int bd, int xd, int r, int (&c)[6]) {
    if constexpr (Wide) {
        // 4 xd <= cw - 1 (the lane has luma samples), so the clamped indices 1 .. 4 lie in dword xd, index 0 in dword
        // xd - 1 or xd, index 5 in dword xd or xd + 1
        const uint32_t* R = reinterpret_cast<const uint32_t*>(P + static_cast<size_t>(r) * st);
        const int i0 = max(4 * xd - 1, 0), i5 = min(4 * xd + 4, cw - 1);
        const uint32_t mid = R[xd], lo = R[i0 >> 2], hi = R[i5 >> 2];
        c[0] = static_cast<int>((lo >> (8 * (i0 & 3))) & 255u);
#pragma unroll
        for (int k = 1; k < 5; k++) {
            const int i = min(4 * xd - 1 + k, cw - 1);
            c[k] = static_cast<int>((mid >> (8 * (i & 3))) & 255u);
        }
        c[5] = static_cast<int>((hi >> (8 * (i5 & 3))) & 255u);
    } else {
#pragma unroll
        for (int k = 0; k < 6; k++) c[k] = k3v_at<Pel>(P, st, cw, ch, bd, 4 * xd - 1 + k, r);
    }
}

// the horizontal sums 3 C[cx] + C[nx] of the lane's 8 luma positions 8 xd + o: cx = 4 xd + (o >> 1) is c[1 + (o >> 1)],
// nx = cx - 1 (o even) or cx + 1 (o odd)
DEVI void k3v_hsum(const int (&c)[6], int (&hs)[8]) {
#pragma unroll
    for (int o = 0; o < 8; o++) {
        const int i = 1 + (o >> 1);
        hs[o] = 3 * c[i] + c[(o & 1) ? i + 1 : i - 1];
    }
}

// luma row y (0 .. h - 1) of a matrix lane: s[o] = Y(8 xd + o, y); wide: the row's two dwords (bytes past w: row
// padding, whose results land in the destination's row padding); plain: x clamped to the plane
template <typename Pel, bool Wide>
DEVI void k3v_luma_row(const Pel* __restrict__ P, int st, int w, int h, int bd, int xd, int y, int (&s)[8]) {
    if constexpr (Wide) {
        const uint32_t* R = reinterpret_cast<const uint32_t*>(P + static_cast<size_t>(y) * st);
        const uint32_t a = R[2 * xd], b = R[2 * xd + 1];
#pragma unroll
        for (int o = 0; o < 4; o++) {
            s[o] = static_cast<int>((a >> (8 * o)) & 255u);
            s[4 + o] = static_cast<int>((b >> (8 * o)) & 255u);
        }
    } else {
#pragma unroll
        for (int o = 0; o < 8; o++) s[o] = k3v_at<Pel>(P, st, w, h, bd, 8 * xd + o, y);
    }
}

// one lane of the matrix class: luma samples 8 xd .. 8 xd + 7 of the rows 2 j - 1 and 2 j, chroma samples
// 4 xd .. 4 xd + 3 of row j
template <typename Pel, bool Wide>
DEVI void k3v_matrix_lane(uint8_t* __restrict__ arena, const h2j_colour& rc, int xd, int j) {
    const int w = rc.w, h = rc.h, cw = w >> 1, ch = h >> 1;
    const int oy = rc.k[0], LY = rc.k[1], LB = rc.k[2], LR = rc.k[3], CB = rc.k[4], CR = rc.k[5], RB = rc.k[6], RR = rc.k[7];
    const Pel* S = reinterpret_cast<const Pel*>(arena + rc.src);
    const Pel* PY = S + rc.src_off[0] + static_cast<size_t>(rc.crop_y) * rc.src_stride[0] + rc.crop_x;
    const Pel* PU = S + rc.src_off[1] + static_cast<size_t>(rc.crop_y >> 1) * rc.src_stride[1] + (rc.crop_x >> 1);
    const Pel* PV = S + rc.src_off[2] + static_cast<size_t>(rc.crop_y >> 1) * rc.src_stride[2] + (rc.crop_x >> 1);
    uint8_t* D = arena + rc.dst;
    const int ra = max(j - 1, 0), rb = min(j, ch - 1);  // the chroma row pair
    int ub[6], vb[6], c[6], ua[8], ubs[8], va[8], vbs[8];
    k3v_chroma_row<Pel, Wide>(PU, rc.src_stride[1], cw, ch, rc.bit_depth_c, xd, ra, c);
    k3v_hsum(c, ua);
    k3v_chroma_row<Pel, Wide>(PV, rc.src_stride[2], cw, ch, rc.bit_depth_c, xd, ra, c);
    k3v_hsum(c, va);
    k3v_chroma_row<Pel, Wide>(PU, rc.src_stride[1], cw, ch, rc.bit_depth_c, xd, rb, ub);
    k3v_hsum(ub, ubs);
    k3v_chroma_row<Pel, Wide>(PV, rc.src_stride[2], cw, ch, rc.bit_depth_c, xd, rb, vb);
    k3v_hsum(vb, vbs);
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int y = 2 * j - 1 + k;  // k = 0: the odd row above (its chroma row is ra), k = 1: the even row (rb)
        if (y < 0 || y >= h) continue;
        int Y[8];
        k3v_luma_row<Pel, Wide>(PY, rc.src_stride[0], w, h, rc.bit_depth, xd, y, Y);
        uint32_t out[2] = {0, 0};
#pragma unroll
        for (int o = 0; o < 8; o++) {
            const int cb16 = k ? ua[o] + 3 * ubs[o] : 3 * ua[o] + ubs[o];
            const int cr16 = k ? va[o] + 3 * vbs[o] : 3 * va[o] + vbs[o];
            const int v = LY * (Y[o] - oy) + LB * (cb16 - 2048) + LR * (cr16 - 2048) + (1 << 19);
            out[o >> 2] |= k3v_clip<20>(v) << (8 * (o & 3));
        }
        uint32_t* q = reinterpret_cast<uint32_t*>(D + rc.dst_off[0] + static_cast<size_t>(y) * rc.dst_stride[0] + 8 * xd);
        q[0] = out[0];
        q[1] = out[1];
    }
    if (j >= ch) return;
    uint32_t ou = 0, ov = 0;  // chroma row j == rb: the samples 4 xd + o are ub[1 + o], vb[1 + o]
#pragma unroll
    for (int o = 0; o < 4; o++) {
        const int db = ub[1 + o] - 128, dr = vb[1 + o] - 128;
        ou |= k3v_clip<16>(CB * db + CR * dr + (128 << 16) + (1 << 15)) << (8 * o);
        ov |= k3v_clip<16>(RB * db + RR * dr + (128 << 16) + (1 << 15)) << (8 * o);
    }
    *reinterpret_cast<uint32_t*>(D + rc.dst_off[1] + static_cast<size_t>(j) * rc.dst_stride[1] + 4 * xd) = ou;
    *reinterpret_cast<uint32_t*>(D + rc.dst_off[2] + static_cast<size_t>(j) * rc.dst_stride[2] + 4 * xd) = ov;
}

// one lane of the range-only class: samples 4 xd .. 4 xd + 3 of the rows y0 .. y0 + H2J_K3V_ROWS - 1 of plane c
template <typename Pel, bool Wide>
DEVI void k3v_range_lane(uint8_t* __restrict__ arena, const h2j_colour& rc, int c, int xd, int y0) {
    const int shc = c ? 1 : 0;
    const int w = rc.w >> shc, h = rc.h >> shc;
    const int st = rc.src_stride[c], bd = c ? rc.bit_depth_c : rc.bit_depth;
    const Pel* P = reinterpret_cast<const Pel*>(arena + rc.src) + rc.src_off[c] + static_cast<size_t>(rc.crop_y >> shc) * st + (rc.crop_x >> shc);
    uint8_t* O = arena + rc.dst + rc.dst_off[c] + 4 * xd;
    // luma: (LY (Y - oy) + 2^19) >> 20; chroma: (M (C - 128) + (128 << 16) + 2^15) >> 16, M = CB or RR
    const int m = c == 0 ? rc.k[1] : (c == 1 ? rc.k[4] : rc.k[7]), o0 = c == 0 ? rc.k[0] : 128;
#pragma unroll
    for (int r = 0; r < H2J_K3V_ROWS; r++) {
        const int y = y0 + r;
        if (y >= h) break;
        int s[4];
        if constexpr (Wide) {
            const uint32_t d = reinterpret_cast<const uint32_t*>(P + static_cast<size_t>(y) * st)[xd];
#pragma unroll
            for (int o = 0; o < 4; o++) s[o] = static_cast<int>((d >> (8 * o)) & 255u);
        } else {
#pragma unroll
            for (int o = 0; o < 4; o++) s[o] = k3v_at<Pel>(P, st, w, h, bd, 4 * xd + o, y);
        }
        uint32_t out = 0;
#pragma unroll
        for (int o = 0; o < 4; o++) {
            const int v = m * (s[o] - o0);
            out |= (c == 0 ? k3v_clip<20>(v + (1 << 19)) : k3v_clip<16>(v + (128 << 16) + (1 << 15))) << (8 * o);
        }
        *reinterpret_cast<uint32_t*>(O + static_cast<size_t>(y) * rc.dst_stride[c]) = out;
    }
}

template <typename Pel, bool Wide, bool Matrix>
__global__ void __launch_bounds__(256) h2j_k3v_colour(uint8_t* __restrict__ arena, const h2j_colour* __restrict__ cmap) {
    // neighbouring tiles share their chroma halo rows and columns: the XCD-aware order (grid.h), as K3u and K3c
    const GridPos gp = xcd_grid_pos();
    const h2j_colour& rc = cmap[gp.y];
    if ((rc.bit_depth > 8) != (sizeof(Pel) == 2) || (rc.wide != 0) != Wide || (rc.matrix != 0) != Matrix) return;
    // K3 SAO or the scale stage may have summed the unconverted picture's MB variances into a jstat this output owns:
    // the rate control wants those of the converted picture, which K4a sums after this kernel (pic == pic2 in the view)
    if (gp.x == 0 && threadIdx.x == 0) reinterpret_cast<h2j_jstat*>(arena + rc.jstat)->var_sum = 0;
    int t = gp.x;
    if constexpr (Matrix) {
        const int dw = (rc.w + 7) >> 3, tx = (dw + 63) >> 6, rows = (rc.h >> 1) + 1;
        if (t >= tx * ((rows + 3) >> 2)) return;
        const int xd = (t % tx) * 64 + static_cast<int>(threadIdx.x & 63);
        const int j = (t / tx) * 4 + static_cast<int>(threadIdx.x >> 6);
        if (xd >= dw || j >= rows) return;
        k3v_matrix_lane<Pel, Wide>(arena, rc, xd, j);
    } else {
        const int tl = h2j_k3v_plane_tiles(rc.w, rc.h), tc = h2j_k3v_plane_tiles(rc.w >> 1, rc.h >> 1);
        int c = 0;
        if (t >= tl + 2 * tc) return;
        if (t >= tl) {
            t -= tl;
            c = 1;
            if (t >= tc) {
                t -= tc;
                c = 2;
            }
        }
        const int w = rc.w >> (c ? 1 : 0), h = rc.h >> (c ? 1 : 0);
        const int dw = (w + 3) >> 2, tx = (dw + 63) >> 6;
        const int xd = (t % tx) * 64 + static_cast<int>(threadIdx.x & 63);
        const int y0 = ((t / tx) * 4 + static_cast<int>(threadIdx.x >> 6)) * H2J_K3V_ROWS;
        if (xd >= dw || y0 >= h) return;
        k3v_range_lane<Pel, Wide>(arena, rc, c, xd, y0);
    }
}

}  // namespace

namespace h2jgpu {  // defined in h2j_kernels.hip: one error slot for the whole C ABI
extern thread_local char g_err[256];
int check(hipError_t e, const char* what);
}  // namespace h2jgpu
using h2jgpu::check;
using h2jgpu::g_err;

extern "C" int h2j_gpu_colour(const h2j_gpu_batch* b, const h2j_colour* map, const int32_t* first, const int32_t* count,
                              const int32_t* tiles, void* stream) {
    if (!b || b->nframes <= 0) return 0;
    if (!map || !first || !count || !tiles) {
        snprintf(g_err, sizeof(g_err), "h2j_gpu_colour: no map");
        return -1;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    // one launch per class present (2 x source class + work class): grid = the class's largest output x its outputs
    for (int cls = 0; cls < H2J_COLOUR_CLASSES; cls++) {
        if (count[cls] <= 0 || tiles[cls] <= 0) continue;
        const dim3 grid(static_cast<unsigned>(tiles[cls]), static_cast<unsigned>(count[cls]));
        const h2j_colour* m = map + first[cls];
        switch (cls) {
        case 0: hipLaunchKernelGGL((h2j_k3v_colour<uint8_t, true, false>), grid, dim3(256), 0, s, b->arena, m); break;
        case 1: hipLaunchKernelGGL((h2j_k3v_colour<uint8_t, true, true>), grid, dim3(256), 0, s, b->arena, m); break;
        case 2: hipLaunchKernelGGL((h2j_k3v_colour<uint8_t, false, false>), grid, dim3(256), 0, s, b->arena, m); break;
        case 3: hipLaunchKernelGGL((h2j_k3v_colour<uint8_t, false, true>), grid, dim3(256), 0, s, b->arena, m); break;
        case 4: hipLaunchKernelGGL((h2j_k3v_colour<uint16_t, false, false>), grid, dim3(256), 0, s, b->arena, m); break;
        default: hipLaunchKernelGGL((h2j_k3v_colour<uint16_t, false, true>), grid, dim3(256), 0, s, b->arena, m); break;
        }
        if (int rc = check(hipGetLastError(), "h2j_k3v_colour")) return rc;
    }
    return 0;
}
