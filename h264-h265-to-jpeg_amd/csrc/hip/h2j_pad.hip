// K3b: padded output (DESIGN.md "Padded output (K3b)").  A rendition's final 8-bit planes -- what the view of its
// picture part shows K4 -- letterboxed into a canvas of the box's size, out of place: 8-bit planes of their own
// (h2j_pad.dst), which K4 / K5 and K3c then read through the canvas view.  For plane c (luma: bw x bh, the picture part
// w x h at px, py; chroma: everything halved) every byte of the canvas plane's rows, row padding included, is
//   canvas(x, y) = P(x - px, y - py)   where px <= x < px + w and py <= y < py + h
//                = fill[c]             elsewhere
// with P the source plane through K4's 8-bit conversion (min((v + (1 << (bd - 9))) >> (bd - 8), 255)), as in K3u.
//
// A workgroup is 64 dwords of 4 canvas samples x 4 lane rows; a lane makes one aligned dword of H2J_K3B_ROWS
// consecutive rows and stores one dword a row.  The canvas rows hold whole 16-byte groups (h2j_spic_stride) and all
// of their dwords are written, so nothing uninitialised reaches K4.  A workgroup whose 4 x H2J_K3B_ROWS rows lie
// above or below the picture part stores splats and loads nothing (a scalar branch: the rows are the workgroup's);
// so does a lane whose dword lies left or right of it.  Dwords inside the picture part, two forms:
//   wide  (h2j_pad.wide: the 8-bit planes K3s / K3r / K3p / K3u wrote -- 16-byte row groups, no crop): the canvas
//         dword at column 4 xd holds the source bytes 4 xd - p .. 4 xd - p + 3 (p = px, or px / 2 in the chroma):
//         two aligned source dwords, indices clamped to the row's dwords, through a byte funnel shift by p & 3
//         (uniform over the plane).
//   plain (an unscaled frame, a window at any origin, an oriented source; uint8_t or uint16_t): four clamped single
//         samples through the conversion.
// A dword that straddles the picture part's left or right edge -- or both: a picture part narrower than a dword --
// takes the fill byte where its column lies outside, by a byte mask.  Nothing outside the source plane's w x h samples
// (wide: its rows' whole dwords) is read.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "grid.h"
#include "h2j_gpu.h"

#define DEVI __host__ __device__ __forceinline__  // (host too: the lane code can be run and checked on a CPU)

namespace {

DEVI int k3b_to8(int v, int bd) {  // K4's 8-bit conversion (jpeg_sample)
    if (bd > 8) {
        v = (v + (1 << (bd - 9))) >> (bd - 8);
        v = v > 255 ? 255 : v;
    }
    return v;
}

// bytes sh .. sh + 3 of the 8 bytes lo, hi (sh 0..3)
DEVI uint32_t k3b_funnel(uint32_t hi, uint32_t lo, int sh) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, static_cast<uint32_t>(sh));
#else
    return static_cast<uint32_t>(((static_cast<uint64_t>(hi) << 32) | lo) >> (8 * sh));
#endif
}

// the plane (c: 0 luma, 1, 2 chroma) of one record as a lane sees it
struct K3bPlane {
    int w, h;    // the picture part
    int bh;      // canvas rows
    int dw;      // canvas dwords a row (the whole row groups)
    int px, py;  // the picture part's place
    int st, bd;  // source: elements a row, bit depth
    uint32_t splat;
};
DEVI K3bPlane k3b_plane(const h2j_pad& pr, int c) {
    const int shc = c ? 1 : 0;
    K3bPlane q;
    q.w = pr.w >> shc;
    q.h = pr.h >> shc;
    q.bh = pr.bh >> shc;
    q.dw = pr.dst_stride[c] >> 2;
    q.px = pr.px >> shc;
    q.py = pr.py >> shc;
    q.st = pr.src_stride[c];
    q.bd = c ? pr.bit_depth_c : pr.bit_depth;
    q.splat = static_cast<uint32_t>(pr.fill[c] & 255) * 0x01010101u;
    return q;
}

// canvas dword xd of source row sy (0 .. h - 1) of a lane whose dword touches the picture part: the source bytes
// s0 .. s0 + 3 (s0 = 4 xd - px, -3 .. w - 1), the fill byte where s0 + i lies outside 0 .. w - 1
template <typename Pel, bool Wide>
DEVI uint32_t k3b_dword(const Pel* __restrict__ P, const K3bPlane& q, int s0, int sy, uint32_t keep) {
    uint32_t v;
    if constexpr (Wide) {
        const int sdw = (q.w + 3) >> 2;  // the source row's dwords
        const uint32_t* R = reinterpret_cast<const uint32_t*>(P + static_cast<size_t>(sy) * q.st);
        const int a = s0 >> 2;  // (arithmetic: -1 for s0 = -3 .. -1)
        const int ia = a < 0 ? 0 : a, ib = a + 1 < sdw ? a + 1 : sdw - 1;
        v = k3b_funnel(R[ib], R[ia], s0 & 3);
    } else {
        v = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            int x = s0 + i;
            x = x < 0 ? 0 : (x > q.w - 1 ? q.w - 1 : x);
            v |= static_cast<uint32_t>(k3b_to8(static_cast<int>(P[static_cast<size_t>(sy) * q.st + x]), q.bd)) << (8 * i);
        }
    }
    return (v & keep) | (q.splat & ~keep);
}

// one lane: canvas dword xd of the rows y0 .. y0 + H2J_K3B_ROWS - 1 of plane c.  fill_only: the caller knows that
// none of these rows crosses the picture part (uniform over the workgroup)
template <typename Pel, bool Wide>
DEVI void k3b_lane(uint8_t* __restrict__ arena, const h2j_pad& pr, int c, int xd, int y0, bool fill_only) {
    constexpr int R = H2J_K3B_ROWS;
    const K3bPlane q = k3b_plane(pr, c);
    uint8_t* O = arena + pr.dst + pr.dst_off[c] + static_cast<size_t>(y0) * pr.dst_stride[c] + 4 * xd;
    const int s0 = 4 * xd - q.px;
    if (fill_only || s0 <= -4 || s0 >= q.w) {  // above, below, left or right of the picture part: no load
#pragma unroll
        for (int j = 0; j < R; j++) {
            if (y0 + j >= q.bh) break;
            *reinterpret_cast<uint32_t*>(O + static_cast<size_t>(j) * pr.dst_stride[c]) = q.splat;
        }
        return;
    }
    uint32_t keep = 0;  // the bytes of the dword that lie inside the picture part
#pragma unroll
    for (int i = 0; i < 4; i++)
        if (s0 + i >= 0 && s0 + i < q.w) keep |= 0xFFu << (8 * i);
    const int shc = c ? 1 : 0;
    const Pel* P = reinterpret_cast<const Pel*>(arena + pr.src) + pr.src_off[c] + static_cast<size_t>(pr.crop_y >> shc) * q.st + (pr.crop_x >> shc);
#pragma unroll
    for (int j = 0; j < R; j++) {
        const int y = y0 + j;
        if (y >= q.bh) break;
        const int sy = y - q.py;
        const uint32_t out = (sy >= 0 && sy < q.h) ? k3b_dword<Pel, Wide>(P, q, s0, sy, keep) : q.splat;
        *reinterpret_cast<uint32_t*>(O + static_cast<size_t>(j) * pr.dst_stride[c]) = out;
    }
}

// thread tid (0 .. 255) of workgroup t (0 .. the grid's width - 1) of one record: its plane, dword and rows
template <typename Pel, bool Wide>
DEVI void k3b_thread(uint8_t* __restrict__ arena, const h2j_pad& pr, int t, int tid) {
    constexpr int R = H2J_K3B_ROWS;
    const int tl = h2j_k3b_plane_tiles(pr.bw, pr.bh), tc = h2j_k3b_plane_tiles(pr.bw >> 1, pr.bh >> 1);
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
    const int shc = c ? 1 : 0;
    const int dw = pr.dst_stride[c] >> 2, tx = (dw + 63) >> 6, bh = pr.bh >> shc;
    const int band = (t / tx) * 4 * R;  // the workgroup's first row: its rows are band .. band + 4 R - 1
    const bool fill_only = band + 4 * R <= (pr.py >> shc) || band >= (pr.py >> shc) + (pr.h >> shc);
    const int xd = (t % tx) * 64 + (tid & 63);
    const int y0 = band + (tid >> 6) * R;
    if (xd >= dw || y0 >= bh) return;
    k3b_lane<Pel, Wide>(arena, pr, c, xd, y0, fill_only);
}

template <typename Pel, bool Wide>
__global__ void __launch_bounds__(256) h2j_k3b_pad(uint8_t* __restrict__ arena, const h2j_pad* __restrict__ pmap) {
    // the XCD-aware order (grid.h), as K3u: the picture part's tiles read neighbouring source lines
    const GridPos gp = xcd_grid_pos();
    const h2j_pad& pr = pmap[gp.y];
    if ((pr.bit_depth > 8) != (sizeof(Pel) == 2) || (pr.wide != 0) != Wide) return;
    k3b_thread<Pel, Wide>(arena, pr, gp.x, static_cast<int>(threadIdx.x));
}

}  // namespace

namespace h2jgpu {  // defined in h2j_kernels.hip: one error slot for the whole C ABI
extern thread_local char g_err[256];
int check(hipError_t e, const char* what);
}  // namespace h2jgpu
using h2jgpu::check;
using h2jgpu::g_err;

extern "C" int h2j_gpu_pad(const h2j_gpu_batch* b, const h2j_pad* map, const int32_t* first, const int32_t* count,
                           const int32_t* tiles, void* stream) {
    if (!b || b->nframes <= 0) return 0;
    if (!map || !first || !count || !tiles) {
        snprintf(g_err, sizeof(g_err), "h2j_gpu_pad: no map");
        return -1;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    // one launch per source class present: grid = the class's largest canvas x its canvases
    for (int cls = 0; cls < H2J_PAD_CLASSES; cls++) {
        if (count[cls] <= 0 || tiles[cls] <= 0) continue;
        const dim3 grid(static_cast<unsigned>(tiles[cls]), static_cast<unsigned>(count[cls]));
        const h2j_pad* m = map + first[cls];
        switch (cls) {
        case 0: hipLaunchKernelGGL((h2j_k3b_pad<uint8_t, true>), grid, dim3(256), 0, s, b->arena, m); break;
        case 1: hipLaunchKernelGGL((h2j_k3b_pad<uint8_t, false>), grid, dim3(256), 0, s, b->arena, m); break;
        default: hipLaunchKernelGGL((h2j_k3b_pad<uint16_t, false>), grid, dim3(256), 0, s, b->arena, m); break;
        }
        if (int rc = check(hipGetLastError(), "h2j_k3b_pad")) return rc;
    }
    return 0;
}
