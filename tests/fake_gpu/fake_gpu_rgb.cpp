// The host-memory stand-in with the finishing stage (fake_gpu_finish.cpp) and the RGB stage: the same library and
// transcript, and the entry point a kernel library with the stage has (include/h2j_gpu.h h2j_gpu_rgb).  Its
// transcript lines (tests/test_rgb_handover.py):
//   rgb map=+<offset from the staging base> first a,b,c count a,b,c tiles a,b,c
//   px <w> <h> layout <1|2> depth <luma>,<chroma> wide <0|1> crop <x>,<y> pitch <luma>,<chroma>,<chroma> base <dst_base> at <dst_off mod 256> own <1: the pixels are no part of the source>
//       one line per record of the map, in map order
#include "fake_gpu_finish.cpp"

extern "C" {
int h2j_gpu_rgb(const h2j_gpu_batch* b, const h2j_rgb* map, const int32_t* first, const int32_t* count, const int32_t* tiles, void*) {
    fprintf(stderr, "rgb map=+%lld first %d,%d,%d count %d,%d,%d tiles %d,%d,%d\n",
            static_cast<long long>(reinterpret_cast<const uint8_t*>(map) - g_din), first[0], first[1], first[2], count[0], count[1],
            count[2], tiles[0], tiles[1], tiles[2]);
    const int n = count[0] + count[1] + count[2];
    for (int i = 0; i < n; i++) {
        const h2j_rgb& r = map[i];
        fprintf(stderr, "px %d %d layout %d depth %d,%d wide %d crop %d,%d pitch %d,%d,%d base %llu at %llu own %d\n", r.w, r.h, r.layout,
                r.bit_depth, r.bit_depth_c, r.wide, r.crop_x, r.crop_y, r.src_stride[0], r.src_stride[1], r.src_stride[2],
                static_cast<unsigned long long>(r.dst_base), static_cast<unsigned long long>(r.dst_off % 256), r.dst_off != r.src ? 1 : 0);
    }
    return stage("rgb", b);
}
}
