// K3c's lane code on the CPU (tests/test_rgb_k3c_host.py builds this with hipcc, the host code under
// AddressSanitizer and UBSan, and runs it): csrc/hip/h2j_rgb.hip marks its lane functions __host__ __device__, so
// the very code a GPU lane runs is called here for every (xd, j) of an output, in each source class, layout and store
// class.  The arena is one heap block that ends with the output and 64 guard bytes, 64 more in front of it: a store
// outside the output's 3 W H bytes changes a guard byte or trips the sanitizer, a misaligned 16- or 32-bit store
// trips UBSan.  Each case is dumped as (w, h, layout), the source window's 8-bit planes, the pixels; the test compares
// them with tests/rgb_ref.py.
//   k3c_host <directory for the dumps>
#include "h2j_rgb.hip"

#include <cstdlib>
#include <cstring>

namespace h2jgpu {  // what h2j_rgb.hip expects of h2j_kernels.hip
thread_local char g_err[256];
int check(hipError_t, const char*) { return 0; }
}  // namespace h2jgpu

static const char* g_dir = ".";

template <typename Pel, bool Wide>
static int run(int w, int h, int layout, int bd, int cropx, int cropy, int n) {
    // source planes: wide: the output's size with 16-byte row groups; plain: a larger picture the window lies in
    const int pw = Wide ? w : w + cropx + 6, ph = Wide ? h : h + cropy + 4;
    int st[3], off[3];
    size_t po = 0;
    for (int c = 0; c < 3; c++) {
        const int cw = c ? pw / 2 : pw, chh = c ? ph / 2 : ph;
        st[c] = Wide ? ((cw + 15) & ~15) : cw;
        off[c] = static_cast<int>(po);
        po += static_cast<size_t>(st[c]) * chh;
    }
    const size_t guard = 64, dstbytes = static_cast<size_t>(3) * w * h;
    const size_t src_at = 256, dst_at = ((src_at + po * sizeof(Pel) + 255) & ~static_cast<size_t>(255)) + 256;
    const size_t total = dst_at + dstbytes + guard;  // the block ends with the guard: anything further is the sanitizer's
    uint8_t* arena = static_cast<uint8_t*>(malloc(total));
    memset(arena, 0xAB, total);
    srand(static_cast<unsigned>(w * 131 + h * 7 + layout + bd));
    Pel* S = reinterpret_cast<Pel*>(arena + src_at);
    for (size_t i = 0; i < po; i++) S[i] = static_cast<Pel>(rand() % (1 << bd));
    h2j_rgb rc{};
    rc.w = w;
    rc.h = h;
    rc.layout = layout;
    rc.bit_depth = rc.bit_depth_c = bd;
    rc.crop_x = cropx;
    rc.crop_y = cropy;
    rc.wide = Wide;
    rc.src = src_at;
    for (int c = 0; c < 3; c++) {
        rc.src_stride[c] = st[c];
        rc.src_off[c] = off[c];
    }
    rc.dst_off = dst_at;
    const int dw = (w + 3) >> 2, rows = (h >> 1) + 1;
    const bool al4 = (w & 3) == 0;
    for (int j = 0; j < rows; j++)
        for (int xd = 0; xd < dw; xd++) {  // the kernel's dispatch (h2j_k3c_rgb)
            if (layout == 2) {
                if (al4) k3c_lane<Pel, Wide, true, true>(arena, rc, xd, j);
                else k3c_lane<Pel, Wide, true, false>(arena, rc, xd, j);
            } else {
                if (al4) k3c_lane<Pel, Wide, false, true>(arena, rc, xd, j);
                else k3c_lane<Pel, Wide, false, false>(arena, rc, xd, j);
            }
        }
    for (size_t i = 0; i < guard; i++)
        if (arena[dst_at - 1 - i] != 0xAB || arena[dst_at + dstbytes + i] != 0xAB) {
            printf("case %d: a byte outside the output's %zu bytes was written\n", n, dstbytes);
            return 1;
        }
    char name[512];
    snprintf(name, sizeof(name), "%s/c%03d.bin", g_dir, n);
    FILE* f = fopen(name, "wb");
    if (!f) return 1;
    const int hdr[3] = {w, h, layout};
    fwrite(hdr, 4, 3, f);
    for (int c = 0; c < 3; c++) {  // the window's planes through K4's 8-bit conversion: the model's input
        const int cw = c ? w / 2 : w, chh = c ? h / 2 : h, cx = c ? cropx / 2 : cropx, cy = c ? cropy / 2 : cropy;
        for (int y = 0; y < chh; y++)
            for (int x = 0; x < cw; x++) {
                int v = S[off[c] + static_cast<size_t>(y + cy) * st[c] + x + cx];
                if (bd > 8) {
                    v = (v + (1 << (bd - 9))) >> (bd - 8);
                    if (v > 255) v = 255;
                }
                fputc(v, f);
            }
    }
    fwrite(arena + dst_at, 1, dstbytes, f);
    fclose(f);
    free(arena);
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1) g_dir = argv[1];
    // odd sizes, W % 4 == 2 with one and several lanes a row, narrower than a lane row, more than one workgroup's 256
    // columns, the 2 x 2 picture whose clamps all hit one chroma sample
    const int sizes[][2] = {{2, 2}, {4, 2}, {2, 4}, {6, 4}, {18, 10}, {18, 128}, {52, 30}, {64, 64}, {72, 40},
                            {48, 200}, {100, 56}, {258, 6}, {260, 18}, {514, 4}};
    int bad = 0, n = 0;
    for (const auto& s : sizes)
        for (int layout = 1; layout <= 2; layout++) {
            bad |= run<uint8_t, true>(s[0], s[1], layout, 8, 0, 0, n++);      // the planes K3s / K3r / K3p / K3u wrote
            bad |= run<uint8_t, false>(s[0], s[1], layout, 8, 36, 10, n++);   // a window at an unaligned origin
            bad |= run<uint8_t, false>(s[0], s[1], layout, 8, 0, 0, n++);     // an unscaled frame
            bad |= run<uint16_t, false>(s[0], s[1], layout, 10, 2, 6, n++);   // 16-bit samples
        }
    printf("%d cases, %s\n", n, bad ? "FAILED" : "ok");
    return bad;
}
