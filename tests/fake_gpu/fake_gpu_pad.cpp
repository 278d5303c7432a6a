// The host-memory stand-in with every earlier stage (fake_gpu_orient.cpp) and the padding stage: the same library and
// transcript, and the entry point a kernel library with the stage has (include/h2j_gpu.h h2j_gpu_pad).  Its transcript
// lines (tests/test_pad_handover.py):
//   pad map=+<offset from the staging base> first a,b,c count a,b,c tiles a,b,c
//   box <w> <h> in <bw> <bh> at <px>,<py> fill <Y>,<Cb>,<Cr> depth <luma>,<chroma> wide <0|1> crop <x>,<y> pitch <source luma>/<canvas luma>,<chroma>,<chroma> at <plane offsets> src <arena offset> dst <arena offset>
//       one line per record of the map, in map order
#include "fake_gpu_orient.cpp"

extern "C" {
int h2j_gpu_pad(const h2j_gpu_batch* b, const h2j_pad* map, const int32_t* first, const int32_t* count, const int32_t* tiles, void*) {
    fprintf(stderr, "pad map=+%lld first %d,%d,%d count %d,%d,%d tiles %d,%d,%d\n",
            static_cast<long long>(reinterpret_cast<const uint8_t*>(map) - g_din), first[0], first[1], first[2], count[0], count[1],
            count[2], tiles[0], tiles[1], tiles[2]);
    const int n = count[0] + count[1] + count[2];
    for (int i = 0; i < n; i++) {
        const h2j_pad& r = map[i];
        fprintf(stderr, "box %d %d in %d %d at %d,%d fill %d,%d,%d depth %d,%d wide %d crop %d,%d pitch %d/%d,%d,%d at %d,%d,%d src %llu dst %llu\n", r.w,
                r.h, r.bw, r.bh, r.px, r.py, r.fill[0], r.fill[1], r.fill[2], r.bit_depth, r.bit_depth_c, r.wide, r.crop_x, r.crop_y,
                r.src_stride[0], r.dst_stride[0], r.dst_stride[1], r.dst_stride[2], r.dst_off[0], r.dst_off[1], r.dst_off[2],
                static_cast<unsigned long long>(r.src), static_cast<unsigned long long>(r.dst));
    }
    return stage("pad", b);
}
}
