// IDecoder facade — drop-in for the reference's Decoder
// (/root/reference/src/Decoder.cpp:39-53 getInstance, :115-361 H265ToJpeg)
// and Encoder (/root/reference/src/Encoder.cpp:104-362).  Same contract:
// borrowed C-string paths, fresh instance per getInstance(), false + a LOG
// line on any failure, output written with fopen("wb+") + fwrite.
// Differences (documented in DESIGN.md): no probe-decode, no fixed 2 MiB
// output buffer (the reference's writeCallback has no bounds check,
// src/Encoder.cpp:29), decoder-delay streams are handled (the first picture
// is decoded directly), 10-bit input is converted with
// v8 = min(255, (v + 2) >> 2) instead of producing a corrupted JPEG.
#include <algorithm>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "IDecoder.h"
#include "api_ext.h"
#include "h2j.h"
#include "out_opts.h"

void LOG(const char* format, ...) {
    char log[1024] = {0};
    va_list ap;
    va_start(ap, format);
    vsnprintf(log, sizeof(log), format, ap);
    va_end(ap);
    time_t ts;
    time(&ts);
    struct tm tmv;
    localtime_r(&ts, &tmv);  // the reference's localtime() is not thread-safe
    char now[64];
    strftime(now, sizeof(now), "%Y-%m-%d %H:%M:%S", &tmv);
    printf("%s | %s\n", now, log);
}

namespace {

// One engine per visible GPU (H2J_ENGINES overrides the count; engine i runs on device
// i % device count); IDecoder instances are cheap handles.  Concurrent H265ToJpeg calls are
// batched: callers queue their bitstreams, and whichever caller finds engines idle takes
// everything queued, splits it over the idle engines (longest-processing-time first by
// bitstream bytes, the host entropy cost) and runs the parts as h2j_engine_transcode batches
// side by side (host entropy decoding fans out over each engine's thread pool, each GPU sees
// one launch per stage), then hands every caller its JPEG.  A lone caller runs a batch of one;
// a JVM calling through JNI from many threads keeps every GPU of the node busy.
struct Request {
    const uint8_t* data = nullptr;
    size_t size = 0;
    // the options of the picture's renditions: one (all 0: the decoded size; h2j_h265_to_jpeg_mem_scaled,
    // _fit) or several (h2j_h265_to_jpeg_mem_multi, _multi3 .. _multi8); per rendition the JPEG (a raw rendition: its
    // pixels), the output's size and status once the batch ran
    std::vector<h2j_out_opts8> opts{h2j::kPlainOutput8};
    std::vector<std::vector<uint8_t>> jpegs;
    std::vector<int32_t> wh;
    std::vector<int> rstatus;
    int status = 0;  // of the first rendition, which is all a plain caller asks for (-1: the batch did not run)
    std::string error;
    bool done = false;
};

struct EngineSlot {
    h2j_engine* e = nullptr;
    bool busy = false;
};

std::mutex g_mu;
std::condition_variable g_cv;
std::deque<Request*> g_queue;
std::vector<EngineSlot> g_engines;
bool g_engines_init = false;

// create the engines (caller holds g_mu); none when no HIP device is visible
void init_engines_locked() {
    if (g_engines_init) return;
    g_engines_init = true;
    const int ndev = h2j_device_count();
    if (ndev <= 0) return;
    int n = ndev;
    if (const char* env = getenv("H2J_ENGINES")) {
        const int v = atoi(env);
        if (v > 0 && v <= 64) n = v;
    }
    for (int i = 0; i < n; i++) {
        // split the host threads between the engines (each creates a pool of that size)
        h2j_engine* e = h2j_engine_create(i % ndev, -n);
        if (e) {
            EngineSlot slot;
            slot.e = e;
            g_engines.push_back(slot);
        }
    }
}

// LPT partition of `work` into k parts by bitstream bytes (each part keeps queue order)
std::vector<std::vector<Request*>> split_lpt(const std::vector<Request*>& work, int k) {
    std::vector<int> idx(work.size());
    for (size_t i = 0; i < idx.size(); i++) idx[i] = static_cast<int>(i);
    std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return work[a]->size > work[b]->size; });
    std::vector<size_t> load(static_cast<size_t>(k), 0);
    std::vector<int> part(work.size());
    for (int i : idx) {
        const int m = static_cast<int>(std::min_element(load.begin(), load.end()) - load.begin());
        part[i] = m;
        load[m] += work[i]->size + 1;
    }
    std::vector<std::vector<Request*>> out(static_cast<size_t>(k));
    for (size_t i = 0; i < work.size(); i++) out[part[i]].push_back(work[i]);
    return out;
}

// run one batch (caller holds no lock); fills jpegs / rstatus / status / error of each request.  Every
// picture is decoded once (h2j::submit_multi8, the transcode form; a plain request is an item with one rendition)
void run_batch(h2j_engine* e, std::vector<Request*>& batch) {
    const int n = static_cast<int>(batch.size());
    if (n == 0) return;
    std::vector<const uint8_t*> ptrs(n);
    std::vector<size_t> sizes(n);
    std::vector<int32_t> nrend(n);
    std::vector<int> base(n + 1, 0);
    std::vector<h2j_out_opts8> opts;
    size_t cap = 8u << 20;
    for (int i = 0; i < n; i++) {
        const Request* q = batch[i];
        ptrs[i] = q->data;
        sizes[i] = q->size;
        nrend[i] = static_cast<int32_t>(q->opts.size());
        base[i + 1] = base[i] + nrend[i];
        opts.insert(opts.end(), q->opts.begin(), q->opts.end());
        cap += (q->size * 4 + (2u << 20)) * static_cast<size_t>(nrend[i]);
    }
    const int total = base[n];
    std::vector<size_t> off(total), len(total);
    std::vector<int> status(total);
    std::vector<int32_t> wh(2 * static_cast<size_t>(total));
    std::vector<uint8_t> out;
    int r = -1;
    for (int attempt = 0; attempt < 3; attempt++) {
        out.resize(cap);
        r = static_cast<int>(h2j::submit_multi8(e, n, ptrs.data(), sizes.data(), nrend.data(), opts.data(), out.data(), cap, off.data(),
                                                len.data(), status.data(), wh.data(), true));
        bool small = false;
        size_t raw = 0;  // what the raw renditions need, exactly
        for (int i = 0; i < total; i++) {
            small = small || status[i] == -50;
            if (opts[i].format) raw += 3 * static_cast<size_t>(wh[2 * i]) * static_cast<size_t>(wh[2 * i + 1]);
        }
        if (!small) break;
        cap = cap * 4 + raw;
    }
    for (int i = 0; i < n; i++) {
        Request* q = batch[i];
        q->jpegs.assign(static_cast<size_t>(nrend[i]), std::vector<uint8_t>());
        q->rstatus.assign(static_cast<size_t>(nrend[i]), 0);
        q->wh.assign(wh.begin() + 2 * base[i], wh.begin() + 2 * base[i + 1]);
        for (int k = 0; k < nrend[i]; k++) {
            const int o = base[i] + k;
            int st = status[o];
            if (r != 0 && st == 0) st = r;
            if (st == 0) {
                q->jpegs[k].assign(out.begin() + static_cast<long>(off[o]), out.begin() + static_cast<long>(off[o] + len[o]));
            } else if (q->error.empty()) {
                const char* m = status[o] != 0 ? h2j_engine_frame_error(e, o) : "";
                q->error = (m && *m) ? m : h2j_engine_error(e);
            }
            q->rstatus[k] = st;
        }
        q->status = q->rstatus[0];
    }
}

// transcode pictures through the shared, batching engines (all of `reqs` join the same queue,
// so a caller's own batch runs together with whatever else is queued)
void transcode_shared_many(const std::vector<Request*>& reqs) {
    std::unique_lock<std::mutex> lk(g_mu);
    init_engines_locked();
    if (g_engines.empty()) {
        for (Request* q : reqs) {
            q->status = -1;
            q->error = "no HIP device available: the MI355X pipeline cannot run";
            q->done = true;
        }
        return;
    }
    for (Request* r : reqs) g_queue.push_back(r);
    auto all_done = [&] {
        for (Request* r : reqs)
            if (!r->done) return false;
        return true;
    };
    while (!all_done()) {
        std::vector<int> idle;
        for (size_t i = 0; i < g_engines.size(); i++)
            if (!g_engines[i].busy) idle.push_back(static_cast<int>(i));
        if (idle.empty() || g_queue.empty()) {
            g_cv.wait(lk);
            continue;
        }
        std::vector<Request*> work(g_queue.begin(), g_queue.end());
        g_queue.clear();
        const int k = static_cast<int>(std::min(idle.size(), work.size()));
        std::vector<std::vector<Request*>> parts = split_lpt(work, k);
        for (int j = 0; j < k; j++) g_engines[idle[j]].busy = true;
        lk.unlock();
        std::vector<std::thread> helpers;
        for (int j = 1; j < k; j++)
            helpers.emplace_back([&, j] { run_batch(g_engines[idle[j]].e, parts[j]); });
        run_batch(g_engines[idle[0]].e, parts[0]);
        for (auto& t : helpers) t.join();
        lk.lock();
        for (Request* q : work) q->done = true;
        for (int j = 0; j < k; j++) g_engines[idle[j]].busy = false;
        g_cv.notify_all();
    }
}

bool transcode_shared(Request& req) {
    transcode_shared_many(std::vector<Request*>{&req});
    return req.status == 0;
}

bool read_file(const char* path, std::vector<uint8_t>& buf) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    if (fseek(f, 0, SEEK_END) != 0) { fclose(f); return false; }
    long n = ftell(f);
    if (n < 0) { fclose(f); return false; }
    rewind(f);
    buf.resize(static_cast<size_t>(n));
    size_t got = n ? fread(buf.data(), 1, static_cast<size_t>(n), f) : 0;
    fclose(f);
    return got == static_cast<size_t>(n);
}

class Decoder : public IDecoder {
public:
    Decoder() { LOG("%s", __PRETTY_FUNCTION__); }
    ~Decoder() override = default;
    bool H265ToJpeg(const char* inputFilePath, const char* outputFilePath) override;
};

bool Decoder::H265ToJpeg(const char* const in, const char* const out) {
    if (in == nullptr || out == nullptr || strlen(in) == 0 || strlen(out) == 0) {
        LOG("input or output path is empty: input:%s, output:%s", in ? in : "(null)", out ? out : "(null)");
        return false;
    }
    std::vector<uint8_t> data;
    if (!read_file(in, data)) {
        LOG("cannot open input file: %s", in);
        return false;
    }
    Request req;
    req.data = data.data();
    req.size = data.size();
    if (!transcode_shared(req)) {
        LOG("transcode failed (%d): %s", req.status, req.error.c_str());
        return false;
    }
    const std::vector<uint8_t>& jpeg = req.jpegs[0];
    FILE* f = fopen(out, "wb+");
    if (!f) {
        LOG("failed to encode Yuv to Jpeg: cannot open %s", out);
        return false;
    }
    size_t w = fwrite(jpeg.data(), 1, jpeg.size(), f);
    fclose(f);
    if (w != jpeg.size()) {
        LOG("failed to write Jpeg file %s", out);
        return false;
    }
    LOG("saved Jpeg data to file %s", out);
    return true;
}

}  // namespace

std::shared_ptr<IDecoder> IDecoder::getInstance() { return std::make_shared<Decoder>(); }

// ---- in-memory and batch entry points beside IDecoder

extern "C" int h2j_h265_to_jpeg_mem(const uint8_t* data, size_t size, uint8_t** jpeg, size_t* jpeg_len) {
    return h2j_h265_to_jpeg_mem_scaled(data, size, 0, 0, jpeg, jpeg_len);
}

static int to_jpeg_mem(const uint8_t* data, size_t size, const h2j_out_opts2& opts, uint8_t** jpeg, size_t* jpeg_len) {
    if (!jpeg || !jpeg_len) return -1;
    *jpeg = nullptr;
    *jpeg_len = 0;
    if (!data || size == 0) return -1;
    Request req;
    req.data = data;
    req.size = size;
    req.opts[0] = h2j::to_opts8(opts);
    if (!transcode_shared(req)) {
        LOG("transcode failed (%d): %s", req.status, req.error.c_str());
        return req.status ? req.status : -1;
    }
    const std::vector<uint8_t>& got = req.jpegs[0];
    uint8_t* p = static_cast<uint8_t*>(malloc(got.size()));
    if (!p) return -1;
    std::memcpy(p, got.data(), got.size());
    *jpeg = p;
    *jpeg_len = got.size();
    return 0;
}

extern "C" int h2j_h265_to_jpeg_mem_scaled(const uint8_t* data, size_t size, int scale_log2, int max_dim, uint8_t** jpeg,
                                           size_t* jpeg_len) {
    return to_jpeg_mem(data, size, h2j_out_opts2{scale_log2, max_dim, 0, 0, 0, {0, 0, 0}}, jpeg, jpeg_len);
}

extern "C" int h2j_h265_to_jpeg_mem_fit(const uint8_t* data, size_t size, int fit_w, int fit_h, int flags, uint8_t** jpeg,
                                        size_t* jpeg_len) {
    return to_jpeg_mem(data, size, h2j_out_opts2{0, 0, fit_w, fit_h, flags, {0, 0, 0}}, jpeg, jpeg_len);
}

// h2j_h265_to_jpeg_mem_multi8 (libH265ToJpegExt.so, api_ext.h), and what every older mem_multi call runs on
int h2j::mem_multi8(const uint8_t* data, size_t size, int nrend, const h2j_out_opts8* opts, uint8_t** jpeg, size_t* jpeg_len, int* status,
                    int32_t* out_wh) {
    if (nrend < 1 || nrend > H2J_MAX_RENDITIONS) return H2J_ERR_RENDITIONS;
    if (!jpeg || !jpeg_len || !status || !opts) return -1;
    for (int r = 0; out_wh && r < 2 * nrend; r++) out_wh[r] = 0;
    for (int r = 0; r < nrend; r++) {
        jpeg[r] = nullptr;
        jpeg_len[r] = 0;
        status[r] = -1;
    }
    if (!data || size == 0) return -1;
    Request req;
    req.data = data;
    req.size = size;
    req.opts.assign(opts, opts + nrend);
    transcode_shared(req);
    if (req.rstatus.size() != static_cast<size_t>(nrend)) {  // the batch did not run (no HIP device)
        LOG("transcode failed (%d): %s", req.status, req.error.c_str());
        return req.status ? req.status : -1;
    }
    for (int r = 0; out_wh && r < 2 * nrend && r < static_cast<int>(req.wh.size()); r++) out_wh[r] = req.wh[r];
    for (int r = 0; r < nrend; r++) {
        status[r] = req.rstatus[r];
        if (status[r] != 0) continue;
        uint8_t* p = static_cast<uint8_t*>(malloc(std::max<size_t>(1, req.jpegs[r].size())));
        if (!p) {
            status[r] = -1;
            continue;
        }
        std::memcpy(p, req.jpegs[r].data(), req.jpegs[r].size());
        jpeg[r] = p;
        jpeg_len[r] = req.jpegs[r].size();
    }
    return 0;
}

// the multi calls on items of any older option type T
template <typename T>
static int to_jpeg_mem_multi(const uint8_t* data, size_t size, int nrend, const T* opts, uint8_t** jpeg, size_t* jpeg_len, int* status,
                             int32_t* out_wh = nullptr) {
    if (nrend < 1 || nrend > H2J_MAX_RENDITIONS) return H2J_ERR_RENDITIONS;
    if (!opts) return -1;
    return h2j::mem_multi8(data, size, nrend, h2j::to_opts8(nrend, opts).data(), jpeg, jpeg_len, status, out_wh);
}

// h2j_h265_to_jpeg_mem_multi7 (libH265ToJpegExt.so, api_ext.h)
int h2j::mem_multi7(const uint8_t* data, size_t size, int nrend, const h2j_out_opts7* opts, uint8_t** jpeg, size_t* jpeg_len, int* status,
                    int32_t* out_wh) {
    if (nrend >= 1 && nrend <= H2J_MAX_RENDITIONS && (!jpeg || !jpeg_len || !status)) return -1;
    return to_jpeg_mem_multi(data, size, nrend, opts, jpeg, jpeg_len, status, out_wh);
}

extern "C" int h2j_h265_to_jpeg_mem_multi6(const uint8_t* data, size_t size, int nrend, const h2j_out_opts6* opts, uint8_t** jpeg,
                                           size_t* jpeg_len, int* status, int32_t* out_wh) {
    if (nrend >= 1 && nrend <= H2J_MAX_RENDITIONS && (!jpeg || !jpeg_len || !status)) return -1;
    return to_jpeg_mem_multi(data, size, nrend, opts, jpeg, jpeg_len, status, out_wh);
}

extern "C" int h2j_h265_to_jpeg_mem_multi(const uint8_t* data, size_t size, int nrend, const h2j_out_opts2* opts, uint8_t** jpeg,
                                          size_t* jpeg_len, int* status) {
    return to_jpeg_mem_multi(data, size, nrend, opts, jpeg, jpeg_len, status);
}
extern "C" int h2j_h265_to_jpeg_mem_multi3(const uint8_t* data, size_t size, int nrend, const h2j_out_opts3* opts, uint8_t** jpeg,
                                           size_t* jpeg_len, int* status) {
    return to_jpeg_mem_multi(data, size, nrend, opts, jpeg, jpeg_len, status);
}
extern "C" int h2j_h265_to_jpeg_mem_multi4(const uint8_t* data, size_t size, int nrend, const h2j_out_opts4* opts, uint8_t** jpeg,
                                           size_t* jpeg_len, int* status) {
    return to_jpeg_mem_multi(data, size, nrend, opts, jpeg, jpeg_len, status);
}
extern "C" int h2j_h265_to_jpeg_mem_multi5(const uint8_t* data, size_t size, int nrend, const h2j_out_opts5* opts, uint8_t** jpeg,
                                           size_t* jpeg_len, int* status) {
    return to_jpeg_mem_multi(data, size, nrend, opts, jpeg, jpeg_len, status);
}

extern "C" void h2j_free(void* p) { free(p); }

extern "C" int h2j_h265_to_jpeg_batch(const char* const* in_paths, const char* const* out_paths, int n, int* ok) {
    if (n <= 0 || !in_paths || !out_paths) return 0;
    std::vector<std::vector<uint8_t>> data(static_cast<size_t>(n));
    std::vector<Request> reqs(static_cast<size_t>(n));
    std::vector<Request*> live;
    for (int i = 0; i < n; i++) {
        if (ok) ok[i] = 0;
        const char* in = in_paths[i];
        const char* out = out_paths[i];
        if (!in || !out || !*in || !*out) {
            LOG("input or output path is empty: input:%s, output:%s", in ? in : "(null)", out ? out : "(null)");
            continue;
        }
        if (!read_file(in, data[i])) {
            LOG("cannot open input file: %s", in);
            continue;
        }
        reqs[i].data = data[i].data();
        reqs[i].size = data[i].size();
        live.push_back(&reqs[i]);
    }
    if (!live.empty()) transcode_shared_many(live);
    int good = 0;
    for (int i = 0; i < n; i++) {
        const Request& q = reqs[i];
        if (!q.done) continue;
        if (q.status != 0) {
            LOG("transcode failed (%d) for %s: %s", q.status, in_paths[i], q.error.c_str());
            continue;
        }
        FILE* f = fopen(out_paths[i], "wb+");
        if (!f) {
            LOG("failed to encode Yuv to Jpeg: cannot open %s", out_paths[i]);
            continue;
        }
        const std::vector<uint8_t>& jpeg = q.jpegs[0];
        const size_t w = fwrite(jpeg.data(), 1, jpeg.size(), f);
        fclose(f);
        if (w != jpeg.size()) {
            LOG("failed to write Jpeg file %s", out_paths[i]);
            continue;
        }
        if (ok) ok[i] = 1;
        good++;
    }
    return good;
}
