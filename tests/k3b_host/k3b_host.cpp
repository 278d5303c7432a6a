// K3b's lane code on the CPU (tests/test_pad_k3b_host.py builds this with hipcc, the host code under
// AddressSanitizer and UBSan, and runs it): csrc/hip/h2j_pad.hip marks its lane functions __host__ __device__, so the
// very code a GPU thread runs (k3b_thread: workgroup and thread index -> plane, dword and rows) is called here for every
// thread of every workgroup of a record's grid, in each source class.  The source planes are a heap block of exactly
// their bytes, so a load even one byte outside them trips the sanitizer; the canvas lies in a block of its own between
// 64 guard bytes with nothing behind, so a store outside it is found in a guard afterwards or trips the sanitizer; a
// misaligned 32-bit access trips UBSan.  The canvas starts as 0xCD: a byte no thread wrote -- row padding included -- shows.  Each case is
// dumped as (w, h, bw, bh, px, py, fill Y, Cb, Cr), the source window's 8-bit planes, the canvas planes without their
// row padding; the test compares them with tests/pad_ref.py.
//   k3b_host <directory for the dumps>
#include "h2j_pad.hip"

#include <cstdlib>
#include <cstring>

namespace h2jgpu {  // what h2j_pad.hip expects of h2j_kernels.hip
thread_local char g_err[256];
int check(hipError_t, const char*) { return 0; }
}  // namespace h2jgpu

static const char* g_dir = ".";

struct Case {
    int w, h, bw, bh, px, py;
};

template <typename Pel, bool Wide>
static int run(const Case& k, int bd, int cropx, int cropy, const int (&fill)[3], int n) {
    // source planes: wide: the picture part's size with 16-byte row groups; plain: a larger picture the window lies in
    const int pw = Wide ? k.w : k.w + cropx + 6, ph = Wide ? k.h : k.h + cropy + 4;
    const size_t guard = 64;
    h2j_pad pr{};
    size_t so = 0, po = 0;
    for (int c = 0; c < 3; c++) {
        const int cw = c ? pw / 2 : pw, chh = c ? ph / 2 : ph;
        pr.src_stride[c] = Wide ? ((cw + 15) & ~15) : cw;
        pr.src_off[c] = static_cast<int32_t>(so);
        so += static_cast<size_t>(pr.src_stride[c]) * chh;
        pr.dst_stride[c] = h2j_spic_stride(c ? k.bw / 2 : k.bw);
        pr.dst_off[c] = static_cast<int32_t>(po);
        po += static_cast<size_t>(pr.dst_stride[c]) * (c ? k.bh / 2 : k.bh);
    }
    // two blocks: the source planes alone (reads leave no trace in a guard: the block's ends are the planes' ends), and
    // [guard][canvas][guard] and nothing more; the arena the lane code sees is the lower block's start
    // (malloc: 16-byte aligned, which is all the dword accesses need)
    uint8_t* sblk = static_cast<uint8_t*>(malloc(so * sizeof(Pel)));
    uint8_t* dblk = static_cast<uint8_t*>(malloc(2 * guard + po));
    memset(dblk, 0xCD, 2 * guard + po);
    uint8_t* arena = sblk < dblk ? sblk : dblk;
    pr.src = static_cast<uint64_t>(sblk - arena);
    pr.dst = static_cast<uint64_t>(dblk + guard - arena);
    srand(static_cast<unsigned>(k.w * 131 + k.h * 7 + k.px + bd));
    Pel* S = reinterpret_cast<Pel*>(sblk);
    for (size_t i = 0; i < so; i++) S[i] = static_cast<Pel>(rand() % (1 << bd));
    pr.w = k.w;
    pr.h = k.h;
    pr.bw = k.bw;
    pr.bh = k.bh;
    pr.px = k.px;
    pr.py = k.py;
    for (int c = 0; c < 3; c++) pr.fill[c] = fill[c];
    pr.bit_depth = pr.bit_depth_c = bd;
    pr.crop_x = cropx;
    pr.crop_y = cropy;
    pr.wide = Wide;
    const int tiles = h2j_k3b_tiles(k.bw, k.bh);
    for (int t = 0; t < tiles + 1; t++)  // (one workgroup more than the record needs: a class's grid is its largest canvas's)
        for (int tid = 0; tid < 256; tid++) k3b_thread<Pel, Wide>(arena, pr, t, tid);
    int bad = 0;
    for (size_t i = 0; i < guard; i++)
        if (dblk[i] != 0xCD || dblk[guard + po + i] != 0xCD) bad = 1;
    if (bad) printf("case %d: a byte outside the canvas's %zu bytes was written\n", n, po);
    const uint8_t* D = dblk + guard;
    for (int c = 0; c < 3 && !bad; c++) {  // the row padding holds the fill byte
        const int cw = c ? k.bw / 2 : k.bw, chh = c ? k.bh / 2 : k.bh;
        for (int y = 0; y < chh; y++)
            for (int x = cw; x < pr.dst_stride[c]; x++)
                if (D[pr.dst_off[c] + static_cast<size_t>(y) * pr.dst_stride[c] + x] != fill[c]) bad = 1;
        if (bad) printf("case %d: row padding of plane %d is not the fill byte\n", n, c);
    }
    char name[512];
    snprintf(name, sizeof(name), "%s/c%03d.bin", g_dir, n);
    FILE* f = fopen(name, "wb");
    if (!f) return 1;
    const int hdr[9] = {k.w, k.h, k.bw, k.bh, k.px, k.py, fill[0], fill[1], fill[2]};
    fwrite(hdr, 4, 9, f);
    for (int c = 0; c < 3; c++) {  // the window's planes through K4's 8-bit conversion: the model's input
        const int cw = c ? k.w / 2 : k.w, chh = c ? k.h / 2 : k.h, cx = c ? cropx / 2 : cropx, cy = c ? cropy / 2 : cropy;
        for (int y = 0; y < chh; y++)
            for (int x = 0; x < cw; x++) {
                int v = S[pr.src_off[c] + static_cast<size_t>(y + cy) * pr.src_stride[c] + x + cx];
                if (bd > 8) {
                    v = (v + (1 << (bd - 9))) >> (bd - 8);
                    if (v > 255) v = 255;
                }
                fputc(v, f);
            }
    }
    for (int c = 0; c < 3; c++) {
        const int cw = c ? k.bw / 2 : k.bw, chh = c ? k.bh / 2 : k.bh;
        for (int y = 0; y < chh; y++) fwrite(D + pr.dst_off[c] + static_cast<size_t>(y) * pr.dst_stride[c], 1, static_cast<size_t>(cw), f);
    }
    fclose(f);
    free(sblk);
    free(dblk);
    return bad;
}

int main(int argc, char** argv) {
    if (argc > 1) g_dir = argv[1];
    // the placements of tests/test_gpu_pad.py (the rule's), then placements of a kind the rule never gives -- the kernel
    // takes any even place inside the canvas: every p & 3 in the luma and the chroma with a picture part narrower than
    // a dword, of one dword and of several, at the canvas's first and last columns and rows
    const Case cases[] = {
        {64, 64, 70, 66, 2, 0}, {64, 64, 78, 66, 6, 0}, {64, 64, 90, 70, 12, 2}, {64, 38, 100, 60, 18, 10}, {50, 26, 50, 50, 0, 12},
        {2, 16, 16, 16, 6, 0}, {24, 100, 46, 100, 10, 0}, {24, 100, 50, 100, 12, 0}, {24, 100, 54, 100, 14, 0}, {6, 2, 6, 6, 0, 2},
        {146, 256, 256, 256, 54, 0}, {128, 84, 128, 128, 0, 22}, {320, 180, 400, 200, 40, 10}, {72, 40, 80, 48, 4, 4},
        {640, 360, 640, 640, 0, 140},
        {2, 2, 16, 4, 0, 0}, {2, 2, 16, 4, 2, 2}, {2, 2, 16, 4, 4, 0}, {2, 2, 16, 4, 6, 2}, {2, 2, 16, 4, 14, 2},
        {4, 2, 20, 36, 0, 34}, {4, 2, 20, 36, 2, 16}, {4, 2, 20, 36, 4, 14}, {4, 2, 20, 36, 6, 0}, {4, 2, 20, 36, 16, 18},
        {18, 20, 300, 22, 0, 2}, {18, 20, 300, 22, 250, 0}, {18, 20, 300, 22, 252, 2}, {18, 20, 300, 22, 254, 0}, {18, 20, 300, 22, 282, 2},
        {258, 4, 600, 4, 342, 0},
    };
    const int fills[][3] = {{114, 128, 128}, {77, 92, 255}, {0, 128, 128}};
    int bad = 0, n = 0, i = 0;
    for (const Case& k : cases) {
        const int(&fill)[3] = fills[i++ % 3];
        bad |= run<uint8_t, true>(k, 8, 0, 0, fill, n++);      // the planes K3s / K3r / K3p / K3u wrote
        bad |= run<uint8_t, false>(k, 8, 36, 10, fill, n++);   // a window at an unaligned origin
        bad |= run<uint8_t, false>(k, 8, 0, 0, fill, n++);     // an unscaled frame
        bad |= run<uint16_t, false>(k, 10, 2, 6, fill, n++);   // 16-bit samples
    }
    printf("%d cases, %s\n", n, bad ? "FAILED" : "ok");
    return bad;
}
