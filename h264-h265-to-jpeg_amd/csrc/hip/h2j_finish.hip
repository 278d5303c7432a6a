// K3u: finishing (DESIGN.md "Finishing (K3u, forced qscale)").  An unsharp mask on the luma of a rendition's
// final 8-bit planes, out of place: the planes the rendition's JPEG source view would otherwise be -> 8-bit
// planes of their own (h2j_finish.dst), which K4 / K5 then read through the view.  For the 8-bit luma plane P
// (h rows x w columns, coordinates clamped to the plane) and strength a = sharpen (1..64, in 1/16):
//   S(x, y) = sum over dy, dx in -1..1 of k[dy][dx] P(x + dx, y + dy),  k = [1 2 1; 2 4 2; 1 2 1]
//   D = 16 P - S
//   out = clip(P + ((a D + 128) >> 8), 0, 255)        (arithmetic shift; |a D| <= 64 * 16 * 255: int32)
// The chroma planes are copied.  A source above 8 bits goes through K4's conversion first
// (min((v + (1 << (bd - 9))) >> (bd - 8), 255)), so P is exactly what K4 would have read.
//
// A workgroup is 64 dwords of 4 output samples x 4 lane rows; a lane makes 4 adjacent outputs of
// H2J_K3U_ROWS consecutive rows and stores one dword a row.  It walks H2J_K3U_ROWS + 2 source rows once, keeping
// the horizontal sums (P(x-1) + 2 P(x) + P(x+1), at most 1020) of the last three.  The destination's rows hold
// whole 16-byte groups (h2j_spic_stride), so the last dword of a row may run into its padding, never past it.
// Source rows, two forms:
//   wide  (h2j_finish.wide: the 8-bit planes K3s / K3r / K3p wrote -- 16-byte row groups, no crop): three
//         aligned dword loads a row, the lane's own and the two beside it (clamped to the row's dwords); the
//         left / right neighbours are the adjacent dwords' bytes, the plane's first and last column replicated
//         by hand (the row padding is not what the clamp wants).
//   plain (an unscaled frame, a window at any origin, an oriented source; uint8_t or uint16_t): six clamped
//         single samples a row through the conversion.
// Nothing outside the source plane's w x h samples (wide: its rows' whole dwords) is read.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "grid.h"
#include "h2j_gpu.h"

#define DEVI __device__ __forceinline__

namespace {

DEVI int k3u_to8(int v, int bd) {  // K4's 8-bit conversion (jpeg_sample)
    if (bd > 8) {
        v = (v + (1 << (bd - 9))) >> (bd - 8);
        v = v > 255 ? 255 : v;
    }
    return v;
}

// row y (clamped) of the lane's window: s[0] = P(x0 - 1), s[1..4] = P(x0 .. x0 + 3), s[5] = P(x0 + 4), clamped
template <typename Pel, bool Wide>
DEVI void k3u_row(const Pel* __restrict__ P, int st, int w, int h, int bd, int xd, int y, int (&s)[6]) {
    y = y < 0 ? 0 : (y > h - 1 ? h - 1 : y);
    if constexpr (Wide) {
        const int dw = (w + 3) >> 2;
        const uint32_t* R = reinterpret_cast<const uint32_t*>(P + static_cast<size_t>(y) * st);
        // Three loads a row, the neighbour dwords being the neighbour lanes' own (they hit in the vector L1).  Taking
        // them from the neighbour lanes by a wave shift (v_mov_b32_dpp wave_shr:1 / wave_shl:1, the wave's end lanes
        // loading theirs) was built and timed: 0.178 against 0.145 ms per 256 960 x 540 outputs, twice each,
        // alternating (profiles/finish_k3u.md) -- slower, and not kept
        const uint32_t c = R[xd], l = R[xd > 0 ? xd - 1 : 0], r = R[xd + 1 < dw ? xd + 1 : dw - 1];
        s[1] = c & 255;
        s[2] = (c >> 8) & 255;
        s[3] = (c >> 16) & 255;
        s[4] = c >> 24;
        s[0] = xd > 0 ? static_cast<int>(l >> 24) : s[1];
        s[5] = static_cast<int>(r & 255);
        // the plane's last column: w is even, so the last dword holds 4 or 2 samples
        // (outputs 2 and 3 of a dword of 2 lie in the destination's row padding)
        const int n = w - 4 * xd;
        if (n == 4) s[5] = s[4];
        if (n == 2) s[3] = s[2];
    } else {
#pragma unroll
        for (int i = 0; i < 6; i++) {
            int x = 4 * xd - 1 + i;
            x = x < 0 ? 0 : (x > w - 1 ? w - 1 : x);
            s[i] = k3u_to8(static_cast<int>(P[static_cast<size_t>(y) * st + x]), bd);
        }
    }
}

template <typename Pel, bool Wide>
__global__ void __launch_bounds__(256) h2j_k3u_finish(uint8_t* __restrict__ arena, const h2j_finish* __restrict__ fmap) {
    constexpr int R = H2J_K3U_ROWS;
    // neighbouring tiles share their halo rows and columns: the XCD-aware order (grid.h), as K3 SAO
    const GridPos gp = xcd_grid_pos();
    const h2j_finish& fr = fmap[gp.y];
    if ((fr.bit_depth > 8) != (sizeof(Pel) == 2) || (fr.wide != 0) != Wide) return;
    // K3 SAO may have summed the unsharpened picture's MB variances into a jstat this output owns: the rate
    // control wants those of the sharpened picture, which K4a sums after this kernel (pic == pic2 in the view)
    if (gp.x == 0 && threadIdx.x == 0) reinterpret_cast<h2j_jstat*>(arena + fr.jstat)->var_sum = 0;
    const int tl = h2j_k3u_plane_tiles(fr.w, fr.h), tc = h2j_k3u_plane_tiles(fr.w >> 1, fr.h >> 1);
    int t = gp.x, c = 0;
    if (t >= tl + 2 * tc) return;
    if (t >= tl) {
        t -= tl;
        c = 1;
        if (t >= tc) {
            t -= tc;
            c = 2;
        }
    }
    const int shc = c ? 1 : 0;
    const int w = fr.w >> shc, h = fr.h >> shc;
    const int dw = (w + 3) >> 2, tx = (dw + 63) >> 6;
    const int xd = (t % tx) * 64 + static_cast<int>(threadIdx.x & 63);
    const int y0 = ((t / tx) * 4 + static_cast<int>(threadIdx.x >> 6)) * R;
    if (xd >= dw || y0 >= h) return;
    const int st = fr.src_stride[c], bd = c ? fr.bit_depth_c : fr.bit_depth;
    const Pel* P = reinterpret_cast<const Pel*>(arena + fr.src) + fr.src_off[c] + static_cast<size_t>(fr.crop_y >> shc) * st + (fr.crop_x >> shc);
    uint8_t* O = arena + fr.dst + fr.dst_off[c] + static_cast<size_t>(y0) * fr.dst_stride[c] + 4 * xd;
    if (c) {  // chroma: copied (converted)
#pragma unroll
        for (int j = 0; j < R; j++) {
            if (y0 + j >= h) break;
            uint32_t out;
            if constexpr (Wide) {
                out = reinterpret_cast<const uint32_t*>(P + static_cast<size_t>(y0 + j) * st)[xd];
            } else {
                out = 0;
#pragma unroll
                for (int o = 0; o < 4; o++) {
                    const int x = min(4 * xd + o, w - 1);
                    out |= static_cast<uint32_t>(k3u_to8(static_cast<int>(P[static_cast<size_t>(y0 + j) * st + x]), bd)) << (8 * o);
                }
            }
            *reinterpret_cast<uint32_t*>(O + static_cast<size_t>(j) * fr.dst_stride[c]) = out;
        }
        return;
    }
    const int a = fr.sharpen;
    int s[6], ha[4], hb[4], pb[4];  // horizontal sums of rows y - 1 and y; the samples of row y
    k3u_row<Pel, Wide>(P, st, w, h, bd, xd, y0 - 1, s);
#pragma unroll
    for (int o = 0; o < 4; o++) ha[o] = s[o] + 2 * s[o + 1] + s[o + 2];
    k3u_row<Pel, Wide>(P, st, w, h, bd, xd, y0, s);
#pragma unroll
    for (int o = 0; o < 4; o++) {
        hb[o] = s[o] + 2 * s[o + 1] + s[o + 2];
        pb[o] = s[o + 1];
    }
#pragma unroll
    for (int j = 0; j < R; j++) {
        if (y0 + j >= h) break;
        k3u_row<Pel, Wide>(P, st, w, h, bd, xd, y0 + j + 1, s);
        uint32_t out = 0;
#pragma unroll
        for (int o = 0; o < 4; o++) {
            const int hc = s[o] + 2 * s[o + 1] + s[o + 2];
            const int S = ha[o] + 2 * hb[o] + hc;
            const int D = 16 * pb[o] - S;
            int v = pb[o] + ((a * D + 128) >> 8);
            v = v < 0 ? 0 : (v > 255 ? 255 : v);
            out |= static_cast<uint32_t>(v) << (8 * o);
            ha[o] = hb[o];
            hb[o] = hc;
            pb[o] = s[o + 1];
        }
        *reinterpret_cast<uint32_t*>(O + static_cast<size_t>(j) * fr.dst_stride[0]) = out;
    }
}

}  // namespace

namespace h2jgpu {  // defined in h2j_kernels.hip: one error slot for the whole C ABI
extern thread_local char g_err[256];
int check(hipError_t e, const char* what);
}  // namespace h2jgpu
using h2jgpu::check;
using h2jgpu::g_err;

extern "C" int h2j_gpu_finish(const h2j_gpu_batch* b, const h2j_finish* map, const int32_t* first, const int32_t* count,
                              const int32_t* tiles, void* stream) {
    if (!b || b->nframes <= 0) return 0;
    if (!map || !first || !count || !tiles) {
        snprintf(g_err, sizeof(g_err), "h2j_gpu_finish: no map");
        return -1;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    // one launch per source class present: grid = the class's largest output x its outputs
    for (int cls = 0; cls < H2J_FINISH_CLASSES; cls++) {
        if (count[cls] <= 0 || tiles[cls] <= 0) continue;
        const dim3 grid(static_cast<unsigned>(tiles[cls]), static_cast<unsigned>(count[cls]));
        const h2j_finish* m = map + first[cls];
        switch (cls) {
        case 0: hipLaunchKernelGGL((h2j_k3u_finish<uint8_t, true>), grid, dim3(256), 0, s, b->arena, m); break;
        case 1: hipLaunchKernelGGL((h2j_k3u_finish<uint8_t, false>), grid, dim3(256), 0, s, b->arena, m); break;
        default: hipLaunchKernelGGL((h2j_k3u_finish<uint16_t, false>), grid, dim3(256), 0, s, b->arena, m); break;
        }
        if (int rc = check(hipGetLastError(), "h2j_k3u_finish")) return rc;
    }
    return 0;
}
