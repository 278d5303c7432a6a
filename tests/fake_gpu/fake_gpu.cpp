// Host-memory stand-in for libh2j_hip.so (include/h2j_gpu.h): no GPU, no kernels.  Allocations are
// calloc, copies are memcpy, streams and events are dummies, every stage returns 0 and runs nothing.
// It writes a transcript of what the engine hands over to stderr (tests/test_engine_handover.py):
//   h2d <bytes> <digest of the staging bytes>      memset <bytes>      d2h <bytes>
//   record #<n>: the n-th event record of the process; wait #<n> and elapsed #<a> #<b> name events by the
//   number of their latest record (0: never recorded), so the transcript shows where each event is recorded,
//   which record a stream waits for and which pairs are timed, whatever index the engine keeps them under
//   <stage> nframes <n> desc <digest of the descriptor, pointers cleared> <pointer>=+<offset from the
//   staging base> | null | set ...
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "h2j_gpu.h"

namespace {

long g_records = 0;               // event records so far
struct Event {
    long record = 0;  // number of its latest record
};
long record_of(void* e) { return e ? static_cast<Event*>(e)->record : 0; }
const uint8_t* g_din = nullptr;  // device side of the last H2D copy: the staging base of the stages that follow

uint64_t fnv(const void* p, size_t n) {
    uint64_t h = 1469598103934665603ull;
    const uint8_t* b = static_cast<const uint8_t*>(p);
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}

__attribute__((constructor)) void hello() { fprintf(stderr, "fake_gpu: host-memory stand-in for libh2j_hip.so\n"); }

// a staging pointer as an offset, then cleared for the digest
template <class T>
void rel(const char* name, const T*& p) {
    if (p) fprintf(stderr, " %s=+%lld", name, static_cast<long long>(reinterpret_cast<const uint8_t*>(p) - g_din));
    else fprintf(stderr, " %s=null", name);
    p = nullptr;
}
template <class T>
void set(const char* name, T*& p) {
    fprintf(stderr, " %s=%s", name, p ? "set" : "null");
    p = nullptr;
}

int stage(const char* name, const h2j_gpu_batch* b) {
    h2j_gpu_batch c;
    memcpy(&c, b, sizeof(c));
    fprintf(stderr, "%s nframes %d", name, c.nframes);
    rel("frames", c.frames); rel("tus", c.tus); rel("coefs", c.coefs); rel("ctbs", c.ctbs); rel("slices", c.slices);
    rel("sl", c.sl); rel("k1map", c.k1map); rel("k1all", c.k1all); rel("sao_map", c.sao_map); rel("k1map8", c.k1map8);
    rel("k1hevc", c.k1hevc); rel("jframes", c.jframes); rel("scale_map", c.scale_map); rel("pyr_map", c.pyr_map);
    set("arena", c.arena); set("seg", c.seg); set("tile_bits", c.tile_bits); set("seg_total", c.seg_total);
    fprintf(stderr, " desc %016llx\n", static_cast<unsigned long long>(fnv(&c, sizeof(c))));
    return 0;
}

}  // namespace

extern "C" {
int h2j_gpu_device_count(void) { return 1; }
int h2j_gpu_set_device(int) { return 0; }
int h2j_gpu_pci_bus_id(int, char*, int) { return -1; }
void* h2j_gpu_malloc(size_t n) { return calloc(1, n ? n : 1); }
int h2j_gpu_free(void* p) { free(p); return 0; }
int h2j_gpu_mem_info(size_t* f, size_t* t) { *f = *t = static_cast<size_t>(256) << 30; return 0; }
void* h2j_gpu_host_alloc(size_t n) { return calloc(1, n ? n : 1); }
int h2j_gpu_host_free(void* p) { free(p); return 0; }
void* h2j_gpu_stream_create(void) { return malloc(1); }
int h2j_gpu_stream_destroy(void* s) { free(s); return 0; }
int h2j_gpu_stream_sync(void*) { return 0; }
int h2j_gpu_memcpy_h2d(void* d, const void* s, size_t n, void*) {
    memcpy(d, s, n);
    g_din = static_cast<const uint8_t*>(d);
    fprintf(stderr, "h2d %zu %016llx\n", n, static_cast<unsigned long long>(fnv(s, n)));
    return 0;
}
int h2j_gpu_memcpy_d2h(void* d, const void* s, size_t n, void*) { memcpy(d, s, n); fprintf(stderr, "d2h %zu\n", n); return 0; }
int h2j_gpu_memset(void* d, int v, size_t n, void*) { memset(d, v, n); fprintf(stderr, "memset %zu\n", n); return 0; }
void* h2j_gpu_event_create(void) { return new Event(); }
int h2j_gpu_event_destroy(void* e) { delete static_cast<Event*>(e); return 0; }
int h2j_gpu_event_record(void* e, void*) {
    if (e) static_cast<Event*>(e)->record = ++g_records;
    fprintf(stderr, "record #%ld\n", record_of(e));
    return 0;
}
int h2j_gpu_stream_wait_event(void*, void* e) { fprintf(stderr, "wait #%ld\n", record_of(e)); return 0; }
float h2j_gpu_event_elapsed_ms(void* a, void* b) { fprintf(stderr, "elapsed #%ld #%ld\n", record_of(a), record_of(b)); return 0; }
const char* h2j_gpu_last_error(void) { return ""; }
int h2j_gpu_recon(const h2j_gpu_batch* b, void*) { return stage("recon", b); }
int h2j_gpu_prep(const h2j_gpu_batch* b, void*) { return stage("prep", b); }
int h2j_gpu_predict(const h2j_gpu_batch* b, void*) { return stage("predict", b); }
int h2j_gpu_prof(unsigned long long*, int, int) { return -1; }
int h2j_gpu_deblock(const h2j_gpu_batch* b, void*) { return stage("deblock", b); }
int h2j_gpu_sao(const h2j_gpu_batch* b, void*) { return stage("sao", b); }
int h2j_gpu_scale(const h2j_gpu_batch* b, void*) { return stage("scale", b); }
int h2j_gpu_jpeg(const h2j_gpu_batch* b, void*) { return stage("jpeg", b); }
int h2j_gpu_histogram(const h2j_gpu_batch* b, void*) { return stage("hist", b); }
int h2j_gpu_entropy(const h2j_gpu_batch* b, void*) { return stage("entropy", b); }
}
