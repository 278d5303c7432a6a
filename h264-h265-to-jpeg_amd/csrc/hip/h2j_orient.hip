// K3o: oriented output (DESIGN.md "Orientation (K3o)").  The cropped planes of a picture's pic2, rotated or
// mirrored into planes of their own (h2j_orient.opic) in the picture's sample type: a permutation of samples,
// no arithmetic.  The K3s / K3r / K3p kernels and K4 then read the oriented planes through a copy of the frame
// (ChunkPlan::wframe), as they read a window.
//
// For an oriented plane O (oh rows x ow columns) of a cropped source plane P (h x w), include/h2j.h:
//   2: O[y][x] = P[y][w-1-x]      3: O[y][x] = P[h-1-y][w-1-x]    4: O[y][x] = P[h-1-y][x]
//   5: O[y][x] = P[x][y]          6: O[y][x] = P[h-1-x][y]        7: O[y][x] = P[h-1-x][w-1-y]
//   8: O[y][x] = P[x][w-1-y]
// i.e. a row flip and a column flip of the source index, after a swap of x and y for 5..8.
//
// The oriented planes are the kernel's own: rows of whole 64-byte groups on 64-byte boundaries
// (h2j_opic_stride), so every store is an aligned 16-byte store that may run into the row's padding and never
// past it.  The source has any alignment (the conformance crop, a mirrored remainder): whole 4- and 16-byte
// groups inside the cropped plane are fetched by loads of their natural width at whatever address (gfx950
// serves unaligned global loads), groups that cross the plane's right or bottom edge sample by sample with
// the index clamped -- nothing outside the cropped plane is read.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>

#include "grid.h"
#include "h2j_gpu.h"

#define DEVI __device__ __forceinline__

namespace {

// Workgroup order: the XCD-aware one (grid.h) -- a picture's neighbouring tiles run on one XCD.  Timed both ways
// on 1024 1080p pictures (profiles/orient_k3o_summary.md, the two builds alternating twice): mirrors 1.03
// against 1.18 ms, transposes 1.28 against 1.53 ms with the dispatcher's own order, unlike the read-once
// streams of grid.h: a tile's rows and its neighbours' share 128-byte lines on both the source and the
// oriented side.  -DH2J_K3O_PLAIN_ORDER builds the dispatcher's order (A/B builds)
DEVI GridPos k3o_grid_pos() {
#ifdef H2J_K3O_PLAIN_ORDER
    return GridPos{static_cast<int>(blockIdx.x), static_cast<int>(blockIdx.y)};
#else
    return xcd_grid_pos();
#endif
}

struct OrientPlane {
    int c, t;        // colour component; workgroup of that plane
    int w, h;        // cropped source plane
    int ow, oh;      // oriented plane
    int sst, dst;    // row pitches in elements
    bool flip_r, flip_c;
};

// the plane workgroup `wg` of record rec works on (false: none -- the grid is the class's largest picture's)
template <typename Pel>
DEVI bool orient_plane(const h2j_frame& f, const h2j_orient& rec, int wg, OrientPlane& p) {
    const bool tr = rec.orient >= 5;
    const int OW = tr ? f.out_h : f.out_w, OH = tr ? f.out_w : f.out_h;
    const int tl = h2j_k3o_plane_tiles(OW, OH, sizeof(Pel), tr), tc = h2j_k3o_plane_tiles(OW >> 1, OH >> 1, sizeof(Pel), tr);
    if (wg >= tl + 2 * tc) return false;
    p.c = 0;
    p.t = wg;
    if (wg >= tl) {
        p.c = 1 + (wg - tl) / tc;
        p.t = (wg - tl) % tc;
    }
    const int sh = p.c ? 1 : 0;
    p.w = f.out_w >> sh;
    p.h = f.out_h >> sh;
    p.ow = OW >> sh;
    p.oh = OH >> sh;
    p.sst = f.pic_stride[p.c];
    p.dst = rec.stride[p.c];
    const int o = rec.orient;
    p.flip_r = o == 3 || o == 4 || o == 6 || o == 7;
    p.flip_c = o == 2 || o == 3 || o == 7 || o == 8;
    return true;
}

template <typename Pel>
DEVI const Pel* orient_src(const h2j_frame& f, const uint8_t* arena, int c) {  // the cropped plane's first sample
    const int sh = c ? 1 : 0;
    return reinterpret_cast<const Pel*>(arena + f.pic2) + f.pic_off[c] + static_cast<size_t>(f.crop_y >> sh) * f.pic_stride[c] +
           (f.crop_x >> sh);
}

// ---- orientations 2, 3, 4: a lane moves one 16-byte segment of an oriented row
template <typename Pel>
DEVI uint4 reverse_samples(uint4 v) {  // the 16 bytes' samples in reverse order
    constexpr uint32_t sel = sizeof(Pel) == 1 ? 0x00010203u : 0x01000302u;  // v_perm_b32: bytes / halfwords of a dword reversed
    return uint4{__builtin_amdgcn_perm(0u, v.w, sel), __builtin_amdgcn_perm(0u, v.z, sel), __builtin_amdgcn_perm(0u, v.y, sel),
                 __builtin_amdgcn_perm(0u, v.x, sel)};
}

template <typename Pel>
__global__ void __launch_bounds__(256) h2j_k3o_mirror(const h2j_frame* __restrict__ frames, uint8_t* __restrict__ arena,
                                                      const h2j_orient* __restrict__ omap) {
    constexpr int N = 16 / static_cast<int>(sizeof(Pel));  // samples of a segment
    const GridPos gp = k3o_grid_pos();
    const h2j_orient& rec = omap[gp.y];
    const h2j_frame& f = frames[rec.frame];
    if (rec.orient < 2 || rec.orient > 4 || (f.bit_depth > 8) != (sizeof(Pel) == 2)) return;
    OrientPlane p;
    if (!orient_plane<Pel>(f, rec, gp.x, p)) return;
    const int spr = (p.ow + N - 1) / N;  // segments of a row
    const int g = p.t * 256 + static_cast<int>(threadIdx.x);
    const int y = g / spr, x0 = (g - y * spr) * N;
    if (y >= p.oh) return;
    const Pel* S = orient_src<Pel>(f, arena, p.c) + static_cast<size_t>(p.flip_r ? p.h - 1 - y : y) * p.sst;
    uint4 v;
    if (x0 + N <= p.w) {  // the whole segment lies in the row: one load, at the mirrored place
        __builtin_memcpy(&v, S + (p.flip_c ? p.w - N - x0 : x0), 16);
        if (p.flip_c) v = reverse_samples<Pel>(v);
    } else {  // the row's last segment: single samples, clamped at the last column (the rest is row padding)
        Pel s[N];
#pragma unroll
        for (int i = 0; i < N; i++) {
            const int x = min(x0 + i, p.w - 1);
            s[i] = S[p.flip_c ? p.w - 1 - x : x];
        }
        __builtin_memcpy(&v, s, 16);
    }
    Pel* D = reinterpret_cast<Pel*>(arena + rec.opic) + rec.off[p.c] + static_cast<size_t>(y) * p.dst + x0;
    *reinterpret_cast<uint4*>(D) = v;
}

// ---- orientations 5 .. 8: a workgroup moves a 64 x 64 tile of the oriented plane through LDS
// A lane loads a 4 x 4 block -- 4 source rows (oriented columns x0 .. x0+3) of 4 samples (oriented rows
// y0 .. y0+3) --, transposes it in registers with v_perm_b32 and writes the 4 oriented row pieces into the
// LDS image of the tile, [oriented row][oriented column].  Lanes run along the source rows (16 lanes x 4
// samples: 64 contiguous samples a row).  After the barrier a lane reads 16 bytes of an oriented row from
// the image and stores them: 4 (8-bit) or 8 (16-bit) neighbouring lanes cover a whole 64-sample row piece.
// The row flip is in the choice of the source rows, the column flip in the order of the transposed pieces.
// LDS pitch: the tile's 16 (32) dwords and one more.  Writes (ds_write_b32, 32 banks over the 32-lane halves):
// a half holds 16 row groups 4 rows apart x 2 columns, bank (4 P yb + xb) mod 32 with P = 17 (33): yb and
// yb + 8 share a bank -- 2-way, which a ds_write_b32 does not pay for (its data path, not the array, sets its
// time).  Reads (4 x ds_read_b32, the pitch is odd): a half holds 8 rows x 4 pieces (4 rows x 8 at 16 bits),
// bank (P row + 4 piece) mod 32: 2-way as well.  A pitch of the bare 16 (32) dwords would put all 16 row
// groups of a write on one bank
template <typename Pel>
struct OrientTile {
    static constexpr int DW = static_cast<int>(sizeof(Pel));  // dwords of 4 samples
    static constexpr int P = 16 * DW + 1;                      // LDS pitch of an oriented row, dwords
    static constexpr int CPR = 4 * DW;                         // 16-byte pieces of a row
};

// 4 rows of 4 samples -> 4 columns of 4 samples (r[i][d], c[k][d]: dword d of row i / column k)
DEVI void transpose4(const uint32_t (&r)[4][1], uint32_t (&c)[4][1]) {
    const uint32_t lo01 = __builtin_amdgcn_perm(r[1][0], r[0][0], 0x05010400u), hi01 = __builtin_amdgcn_perm(r[1][0], r[0][0], 0x07030602u);
    const uint32_t lo23 = __builtin_amdgcn_perm(r[3][0], r[2][0], 0x05010400u), hi23 = __builtin_amdgcn_perm(r[3][0], r[2][0], 0x07030602u);
    c[0][0] = __builtin_amdgcn_perm(lo23, lo01, 0x05040100u);
    c[1][0] = __builtin_amdgcn_perm(lo23, lo01, 0x07060302u);
    c[2][0] = __builtin_amdgcn_perm(hi23, hi01, 0x05040100u);
    c[3][0] = __builtin_amdgcn_perm(hi23, hi01, 0x07060302u);
}
DEVI void transpose4(const uint32_t (&r)[4][2], uint32_t (&c)[4][2]) {
#pragma unroll
    for (int d = 0; d < 2; d++) {  // samples 2d, 2d + 1 of every row
        c[2 * d][0] = __builtin_amdgcn_perm(r[1][d], r[0][d], 0x05040100u);
        c[2 * d][1] = __builtin_amdgcn_perm(r[3][d], r[2][d], 0x05040100u);
        c[2 * d + 1][0] = __builtin_amdgcn_perm(r[1][d], r[0][d], 0x07060302u);
        c[2 * d + 1][1] = __builtin_amdgcn_perm(r[3][d], r[2][d], 0x07060302u);
    }
}

template <typename Pel>
__global__ void __launch_bounds__(256) h2j_k3o_transpose(const h2j_frame* __restrict__ frames, uint8_t* __restrict__ arena,
                                                         const h2j_orient* __restrict__ omap) {
    typedef OrientTile<Pel> T;
    __shared__ uint32_t img[64 * T::P];
    const GridPos gp = k3o_grid_pos();
    const h2j_orient& rec = omap[gp.y];
    const h2j_frame& f = frames[rec.frame];
    if (rec.orient < 5 || rec.orient > 8 || (f.bit_depth > 8) != (sizeof(Pel) == 2)) return;
    OrientPlane p;
    if (!orient_plane<Pel>(f, rec, gp.x, p)) return;
    const int tx = (p.ow + 63) >> 6;
    const int X0 = (p.t % tx) * 64, Y0 = (p.t / tx) * 64;  // the tile in the oriented plane
    const int tid = static_cast<int>(threadIdx.x);
    {
        const int yb = tid & 15, xb = tid >> 4;
        const int x0 = X0 + 4 * xb, y0 = Y0 + 4 * yb;
        const Pel* S = orient_src<Pel>(f, arena, p.c);
        uint32_t r[4][T::DW], c[4][T::DW];
        if (x0 + 3 < p.ow && y0 + 3 < p.oh) {
            const int col = p.flip_c ? p.w - 4 - y0 : y0;  // the 4 source columns, ascending
#pragma unroll
            for (int i = 0; i < 4; i++)
                __builtin_memcpy(r[i], S + static_cast<size_t>(p.flip_r ? p.h - 1 - (x0 + i) : x0 + i) * p.sst + col, 4 * sizeof(Pel));
        } else {  // a block across the plane's right or bottom edge: single samples, clamped (unused ones are not stored)
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int x = min(x0 + i, p.ow - 1);
                const Pel* R = S + static_cast<size_t>(p.flip_r ? p.h - 1 - x : x) * p.sst;
                Pel s[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int y = min(y0 + (p.flip_c ? 3 - k : k), p.oh - 1);
                    s[k] = R[p.flip_c ? p.w - 1 - y : y];
                }
                __builtin_memcpy(r[i], s, 4 * sizeof(Pel));
            }
        }
        transpose4(r, c);
#pragma unroll
        for (int j = 0; j < 4; j++) {  // oriented row y0 + j: source column j, or 3 - j of the ascending four
            uint32_t* d = img + (4 * yb + j) * T::P + xb * T::DW;
#pragma unroll
            for (int q = 0; q < T::DW; q++) d[q] = p.flip_c ? c[3 - j][q] : c[j][q];
        }
    }
    __syncthreads();
    constexpr int N = 16 / static_cast<int>(sizeof(Pel));
#pragma unroll
    for (int m = 0; m < T::CPR / 4; m++) {
        const int ch = tid + 256 * m, yl = ch / T::CPR, q = ch % T::CPR;
        const int y = Y0 + yl, x = X0 + q * N;
        if (y >= p.oh || x >= p.ow) continue;
        const uint32_t* s = img + yl * T::P + 4 * q;
        Pel* D = reinterpret_cast<Pel*>(arena + rec.opic) + rec.off[p.c] + static_cast<size_t>(y) * p.dst + x;
        *reinterpret_cast<uint4*>(D) = uint4{s[0], s[1], s[2], s[3]};
    }
}

}  // namespace

namespace h2jgpu {  // defined in h2j_kernels.hip: one error slot for the whole C ABI
extern thread_local char g_err[256];
int check(hipError_t e, const char* what);
}  // namespace h2jgpu
using h2jgpu::check;
using h2jgpu::g_err;

extern "C" int h2j_gpu_orient(const h2j_gpu_batch* b, const h2j_orient* map, const int32_t* first, const int32_t* count,
                              const int32_t* tiles, void* stream) {
    if (!b || b->nframes <= 0) return 0;
    if (!map || !first || !count || !tiles) {
        snprintf(g_err, sizeof(g_err), "h2j_gpu_orient: no map");
        return -1;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    // one launch per class present (sample type x transposing): grid = the class's largest picture x its pictures
    for (int cls = 0; cls < H2J_ORIENT_CLASSES; cls++) {
        if (count[cls] <= 0 || tiles[cls] <= 0) continue;
        const dim3 grid(static_cast<unsigned>(tiles[cls]), static_cast<unsigned>(count[cls]));
        const h2j_orient* m = map + first[cls];
        switch (cls) {
        case 0: hipLaunchKernelGGL(h2j_k3o_mirror<uint8_t>, grid, dim3(256), 0, s, b->frames, b->arena, m); break;
        case 1: hipLaunchKernelGGL(h2j_k3o_transpose<uint8_t>, grid, dim3(256), 0, s, b->frames, b->arena, m); break;
        case 2: hipLaunchKernelGGL(h2j_k3o_mirror<uint16_t>, grid, dim3(256), 0, s, b->frames, b->arena, m); break;
        default: hipLaunchKernelGGL(h2j_k3o_transpose<uint16_t>, grid, dim3(256), 0, s, b->frames, b->arena, m); break;
        }
        if (int rc = check(hipGetLastError(), (cls & 1) ? "h2j_k3o_transpose" : "h2j_k3o_mirror")) return rc;
    }
    return 0;
}
