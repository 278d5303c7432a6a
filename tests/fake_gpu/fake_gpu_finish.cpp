// The host-memory stand-in (fake_gpu.cpp) with the finishing stage: the same library and transcript, and the
// two entry points a kernel library with the stage has (include/h2j_gpu.h h2j_gpu_finish, h2j_gpu_jpeg2).  Their
// transcript lines (tests/test_finish_api.py):
//   finish map=+<offset from the staging base> first a,b,c count a,b,c tiles a,b,c
//   fin <w> <h> sharpen <a> depth <luma>,<chroma> wide <0|1> crop <x>,<y> pitch <source luma>/<sharpened luma>,<chroma>,<chroma> own <1: dst is no part of src>
//       one line per record of the map, in map order
//   qforce=+<offset from the staging base> <one value per view>, then the jpeg stage line
#include "fake_gpu.cpp"

extern "C" {
int h2j_gpu_finish(const h2j_gpu_batch* b, const h2j_finish* map, const int32_t* first, const int32_t* count, const int32_t* tiles,
                   void*) {
    fprintf(stderr, "finish map=+%lld first %d,%d,%d count %d,%d,%d tiles %d,%d,%d\n",
            static_cast<long long>(reinterpret_cast<const uint8_t*>(map) - g_din), first[0], first[1], first[2], count[0], count[1],
            count[2], tiles[0], tiles[1], tiles[2]);
    const int n = count[0] + count[1] + count[2];
    for (int i = 0; i < n; i++) {
        const h2j_finish& r = map[i];
        fprintf(stderr, "fin %d %d sharpen %d depth %d,%d wide %d crop %d,%d pitch %d/%d,%d,%d own %d\n", r.w, r.h, r.sharpen, r.bit_depth,
                r.bit_depth_c, r.wide, r.crop_x, r.crop_y, r.src_stride[0], r.dst_stride[0], r.dst_stride[1], r.dst_stride[2],
                r.dst != r.src && r.jstat != 0 ? 1 : 0);
    }
    return stage("finish", b);
}
int h2j_gpu_jpeg2(const h2j_gpu_batch* b, const int32_t* qforce, void*) {
    fprintf(stderr, "qforce=+%lld", static_cast<long long>(reinterpret_cast<const uint8_t*>(qforce) - g_din));
    for (int i = 0; i < b->nframes; i++) fprintf(stderr, " %d", qforce[i]);
    fprintf(stderr, "\n");
    return stage("jpeg", b);
}
}
