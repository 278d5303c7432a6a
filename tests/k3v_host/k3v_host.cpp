// K3v's lane code on the CPU (tests/test_colour_k3v_host.py builds this with hipcc, the host code under
// AddressSanitizer and UBSan, and runs it): csrc/hip/h2j_colour.hip marks its lane functions __host__ __device__, so
// the very code a GPU lane runs is called here for every lane of an output, in each of the six classes (source class x
// work class).  The arena is one heap block that ends with the output's planes and 64 guard bytes, 64 more in front of
// them: a store outside the planes' rows (their row padding included) changes a guard byte or trips the sanitizer, a
// misaligned 32-bit store or load trips UBSan, a read outside the arena the sanitizer.  Each case is dumped as
// (w, h, matrix_coefficients, full), the source window's 8-bit planes, the converted planes without their row padding;
// the test compares them with tests/colour_ref.py.
//   k3v_host <directory for the dumps>
#include "h2j_colour.hip"

#include <cstdlib>
#include <cstring>

namespace h2jgpu {  // what h2j_colour.hip expects of h2j_kernels.hip
thread_local char g_err[256];
int check(hipError_t, const char*) { return 0; }
}  // namespace h2jgpu

static const char* g_dir = ".";

// oy, LY, LB, LR, CB, CR, RB, RR (include/h2j.h "Colour"; tests/test_colour_ref.py pins them)
static const int kSets[6][10] = {{6, 0, 16, 1220945, 0, 0, 74606, 0, 0, 74606},
                                 {1, 0, 16, 1220945, 7578, 14628, 73849, -8255, -5405, 73367},
                                 {1, 1, 0, 1048576, 6657, 12850, 64871, -7252, -4748, 64448},
                                 {9, 0, 16, 1220945, 8795, 7872, 74248, -4443, -6273, 72854},
                                 {9, 1, 0, 1048576, 7726, 6915, 65222, -3903, -5511, 63997},
                                 {6, 1, 0, 1048576, 0, 0, 65536, 0, 0, 65536}};

template <typename Pel, bool Wide>
static int run(int w, int h, int set, int bd, int cropx, int cropy, int n) {
    // source planes: wide: the output's size with 16-byte row groups; plain: a larger picture the window lies in
    const int pw = Wide ? w : w + cropx + 6, ph = Wide ? h : h + cropy + 4;
    int st[3], off[3], dst_st[3], dst_off[3];
    size_t po = 0, dpo = 0;
    for (int c = 0; c < 3; c++) {
        const int cw = c ? pw / 2 : pw, chh = c ? ph / 2 : ph;
        st[c] = Wide ? ((cw + 15) & ~15) : cw;
        off[c] = static_cast<int>(po);
        po += static_cast<size_t>(st[c]) * chh;
        dst_st[c] = h2j_spic_stride(c ? w / 2 : w);
        dst_off[c] = static_cast<int>(dpo);
        dpo += static_cast<size_t>(dst_st[c]) * (c ? h / 2 : h);
    }
    const size_t guard = 64;
    const size_t src_at = 256, dst_at = ((src_at + po * sizeof(Pel) + 255) & ~static_cast<size_t>(255)) + 256;
    const size_t jstat_at = 0;  // (the first 256 bytes: the jstat whose var_sum the kernel, not the lane code, clears)
    const size_t total = dst_at + dpo + guard;  // the block ends with the guard: anything further is the sanitizer's
    uint8_t* arena = static_cast<uint8_t*>(malloc(total));
    memset(arena, 0xAB, total);
    srand(static_cast<unsigned>(w * 131 + h * 7 + set + bd));
    Pel* S = reinterpret_cast<Pel*>(arena + src_at);
    for (size_t i = 0; i < po; i++) {
        // a third of the samples at the ends of the range, so that every clip acts
        const int r = rand();
        S[i] = static_cast<Pel>((r & 3) == 0 ? ((r & 4) ? (1 << bd) - 1 - ((r >> 3) % 8) : (r >> 3) % 8) : (r >> 3) % (1 << bd));
    }
    h2j_colour rc{};
    rc.w = w;
    rc.h = h;
    for (int i = 0; i < 8; i++) rc.k[i] = kSets[set][2 + i];
    rc.matrix = (rc.k[2] | rc.k[3] | rc.k[5] | rc.k[6]) ? 1 : 0;
    rc.bit_depth = rc.bit_depth_c = bd;
    rc.crop_x = cropx;
    rc.crop_y = cropy;
    rc.wide = Wide;
    rc.src = src_at;
    rc.dst = dst_at;
    rc.jstat = jstat_at;
    for (int c = 0; c < 3; c++) {
        rc.src_stride[c] = st[c];
        rc.src_off[c] = off[c];
        rc.dst_stride[c] = dst_st[c];
        rc.dst_off[c] = dst_off[c];
    }
    if (rc.matrix) {  // the kernel's dispatch (h2j_k3v_colour)
        const int dw = (w + 7) >> 3, rows = (h >> 1) + 1;
        for (int j = 0; j < rows; j++)
            for (int xd = 0; xd < dw; xd++) k3v_matrix_lane<Pel, Wide>(arena, rc, xd, j);
    } else {
        for (int c = 0; c < 3; c++) {
            const int cw = c ? w / 2 : w, chh = c ? h / 2 : h;
            for (int y0 = 0; y0 < chh; y0 += H2J_K3V_ROWS)
                for (int xd = 0; xd < (cw + 3) >> 2; xd++) k3v_range_lane<Pel, Wide>(arena, rc, c, xd, y0);
        }
    }
    for (size_t i = 0; i < guard; i++)
        if (arena[dst_at - 1 - i] != 0xAB || arena[dst_at + dpo + i] != 0xAB) {
            printf("case %d: a byte outside the output's %zu bytes was written\n", n, dpo);
            return 1;
        }
    char name[512];
    snprintf(name, sizeof(name), "%s/c%03d.bin", g_dir, n);
    FILE* f = fopen(name, "wb");
    if (!f) return 1;
    const int hdr[4] = {w, h, kSets[set][0], kSets[set][1]};
    fwrite(hdr, 4, 4, f);
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
    for (int c = 0; c < 3; c++) {
        const int cw = c ? w / 2 : w, chh = c ? h / 2 : h;
        for (int y = 0; y < chh; y++) fwrite(arena + dst_at + dst_off[c] + static_cast<size_t>(y) * dst_st[c], 1, static_cast<size_t>(cw), f);
    }
    fclose(f);
    free(arena);
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1) g_dir = argv[1];
    // W % 8 = 0, 2, 4, 6 with one and several lanes a row, W % 16 both ways (the row padding), a single chroma row,
    // narrower than a lane, more than one workgroup's 512 (matrix) / 256 (range-only) columns, the 2 x 2 picture
    // whose clamps all hit one chroma sample
    const int sizes[][2] = {{2, 2}, {4, 2}, {2, 4}, {6, 2}, {6, 4}, {8, 8}, {16, 2}, {18, 10}, {18, 128}, {52, 30}, {58, 64}, {60, 64},
                            {62, 64}, {64, 64}, {72, 40}, {48, 200}, {100, 56}, {258, 6}, {260, 18}, {514, 4}, {1030, 4}};
    int bad = 0, n = 0;
    for (const auto& s : sizes)
        for (int set = 0; set < 6; set++) {
            bad |= run<uint8_t, true>(s[0], s[1], set, 8, 0, 0, n++);      // the planes K3s / K3r / K3p wrote
            bad |= run<uint8_t, false>(s[0], s[1], set, 8, 38, 10, n++);   // a window at an unaligned origin (chroma origin 19)
            bad |= run<uint8_t, false>(s[0], s[1], set, 8, 0, 0, n++);     // an unscaled frame
            bad |= run<uint16_t, false>(s[0], s[1], set, 10, 2, 6, n++);   // 16-bit samples
        }
    printf("%d cases, %s\n", n, bad ? "FAILED" : "ok");
    return bad;
}
