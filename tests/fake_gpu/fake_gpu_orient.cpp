// The host-memory stand-in with the finishing and RGB stages (fake_gpu_rgb.cpp) and the orientation stage: the same
// library and transcript, and the entry point a kernel library with the stage has (include/h2j_gpu.h h2j_gpu_orient).
// This is the stand-in with every stage.  Its transcript lines (tests/test_handover_recorded.py):
//   orient map=+<offset from the staging base> first a,b,c,d count a,b,c,d tiles a,b,c,d
//   opic frame <frame> orient <2..8> pitch <luma>,<chroma>,<chroma> at <luma>,<chroma>,<chroma>
//       one line per record of the map, in map order (every field but the arena address)
#include "fake_gpu_rgb.cpp"

extern "C" {
int h2j_gpu_orient(const h2j_gpu_batch* b, const h2j_orient* map, const int32_t* first, const int32_t* count, const int32_t* tiles,
                   void*) {
    fprintf(stderr, "orient map=+%lld first %d,%d,%d,%d count %d,%d,%d,%d tiles %d,%d,%d,%d\n",
            static_cast<long long>(reinterpret_cast<const uint8_t*>(map) - g_din), first[0], first[1], first[2], first[3], count[0],
            count[1], count[2], count[3], tiles[0], tiles[1], tiles[2], tiles[3]);
    const int n = count[0] + count[1] + count[2] + count[3];
    for (int i = 0; i < n; i++) {
        const h2j_orient& r = map[i];
        fprintf(stderr, "opic frame %d orient %d pitch %d,%d,%d at %d,%d,%d\n", r.frame, r.orient, r.stride[0], r.stride[1], r.stride[2],
                r.off[0], r.off[1], r.off[2]);
    }
    return stage("orient", b);
}
}
