// The C ABI of include/h2j.h on the batch engine (engine.h): every entry point that takes an engine, the pure
// option functions (out_opts.h) and the inspection helpers.
#include <cstdlib>
#include <cstring>

#include "api_ext.h"
#include "bitstream.h"
#include "engine.h"
#include "heif.h"
#include "out_opts.h"

using h2j::Engine;
using h2j::Slot;

struct h2j_engine {
    Engine e;
};

// submit one batch; latency: the synchronous plan (small tail chunks), else the throughput plan.
// Item i has nrend[i] renditions (null: one each); opts and the output arrays are item-major over all of
// them (opts null: the decoded size)
static int64_t submit_batch(h2j_engine* w, int n, const uint8_t* const* data, const size_t* sizes, const int32_t* nrend,
                            const h2j_out_opts8* opts, uint8_t* out, size_t out_cap, size_t* out_off, size_t* out_len,
                            int* status, bool latency, int32_t* out_wh = nullptr) {
    Engine& e = w->e;
    std::unique_ptr<h2j::Batch> b(new h2j::Batch());
    b->n = n;
    b->data = data;
    b->sizes = sizes;
    b->out = out;
    b->out_cap = out_cap;
    b->out_off = out_off;
    b->out_len = out_len;
    b->status = status;
    b->out_wh = out_wh;
    b->rbase.assign(static_cast<size_t>(n) + 1, 0);
    for (int i = 0; i < n; i++) b->rbase[i + 1] = b->rbase[i] + (nrend ? nrend[i] : 1);
    b->nout = b->rbase[n];
    if (opts) b->opts.assign(opts, opts + b->nout);
    else b->opts.assign(static_cast<size_t>(b->nout), h2j::kPlainOutput8);
    for (int i = 0; i < b->nout; i++) {
        out_len[i] = 0;
        out_off[i] = 0;
        status[i] = 0;
        if (out_wh) out_wh[2 * i] = out_wh[2 * i + 1] = 0;
    }
    b->bounds = latency ? h2j::chunk_bounds(n) : h2j::chunk_bounds_throughput(n);
    const int nchunks = static_cast<int>(b->bounds.size()) - 1;
    b->chunk_of.assign(static_cast<size_t>(n), 0);
    for (int c = 0; c < nchunks; c++)
        for (int i = b->bounds[c]; i < b->bounds[c + 1]; i++) b->chunk_of[i] = c;
    b->left.reset(new std::atomic<int>[std::max(1, nchunks)]);
    for (int c = 0; c < nchunks; c++) b->left[c] = b->bounds[c + 1] - b->bounds[c];
    e.start_threads();
    std::lock_guard<std::mutex> g(e.amu);
    b->ticket = e.next_ticket++;
    b->t0 = h2j::now_ms();
    const int64_t t = b->ticket;
    e.active++;
    e.parse_q.push_back(b.get());
    e.gpu_q.push_back(b.get());
    e.batches.push_back(std::move(b));
    e.acv.notify_all();
    return t;
}

// nrend[i] in 1..H2J_MAX_RENDITIONS for every item, and options for them
static bool renditions_valid(int n, const int32_t* nrend, const void* opts) {
    if (n < 0 || (n > 0 && (!nrend || !opts))) return false;
    for (int i = 0; i < n; i++)
        if (nrend[i] < 1 || nrend[i] > H2J_MAX_RENDITIONS) return false;
    return true;
}

// the multi calls on items of any option type T: submit, and with `latency` (the transcode form) wait
template <typename T>
static int64_t submit_multi_any(h2j_engine* w, int n, const uint8_t* const* data, const size_t* sizes, const int32_t* nrend, const T* opts,
                                uint8_t* out, size_t out_cap, size_t* out_off, size_t* out_len, int* status, bool latency,
                                int32_t* out_wh = nullptr) {
    if (!w) return -1;
    if (!renditions_valid(n, nrend, opts)) return H2J_ERR_RENDITIONS;
    int total = 0;
    for (int i = 0; i < n; i++) total += nrend[i];
    const int64_t t = submit_batch(w, n, data, sizes, nrend, h2j::to_opts8(total, opts).data(), out, out_cap, out_off, out_len, status, latency, out_wh);
    return latency ? h2j_engine_wait(w, t) : t;
}

// parse one picture into jobs[0] of slot 0, with the outputs of its nrend option sets (valid ones)
static int single_job(h2j_engine* w, const uint8_t* data, size_t size, const h2j_out_opts8* o = &h2j::kPlainOutput8, int nrend = 1) {
    Engine& e = w->e;
    e.quiesce();
    if (h2j_gpu_set_device(e.device)) return e.fail(h2j_gpu_last_error());
    if (e.jobs.empty()) e.jobs.resize(1);
    e.jobs[0].threads = e.pool->size() + 1;  // independent slices on several threads
    int r = h2j::parse_any(data, size, e.jobs[0]);
    if (r) return e.fail("parse failed: " + e.jobs[0].message);
    h2j::resolve_outputs(o, nrend, e.jobs[0]);
    e.jobs[0].out_base = 0;
    e.slot[0].live.assign(1, 0);
    e.slot[0].jobs = &e.jobs;
    return 0;
}

// copy picture k of slot s (after sync) out as uint16 cropped planes
static int copy_planes(Engine& e, Slot& s, int k, int stage, uint16_t* planes_out, size_t cap, int* info) {
    const h2j_frame& f = s.plan.frames[k];
    const int w_ = f.out_w, h_ = f.out_h;
    const size_t need = static_cast<size_t>(w_) * h_ * 3 / 2;
    info[0] = w_;
    info[1] = h_;
    info[2] = f.bit_depth;
    if (cap < need) return e.fail("output buffer too small");
    const size_t pel = f.bit_depth > 8 ? 2 : 1;
    const uint64_t base = stage == 0 ? f.pic2 : f.pic;
    const size_t pic_bytes = static_cast<size_t>(f.width) * f.height * 3 / 2 * pel;
    std::vector<uint8_t> tmp(pic_bytes);
    if (h2j_gpu_memcpy_d2h(tmp.data(), static_cast<uint8_t*>(s.d_arena.p) + base, pic_bytes, s.stream) ||
        h2j_gpu_stream_sync(s.stream))
        return e.fail(h2j_gpu_last_error());
    size_t o = 0;
    for (int c = 0; c < 3; c++) {
        const int sh = c ? 1 : 0;
        const int cw = w_ >> sh, ch = h_ >> sh;
        for (int y = 0; y < ch; y++)
            for (int x = 0; x < cw; x++) {
                const size_t idx = static_cast<size_t>(f.pic_off[c]) +
                                   static_cast<size_t>(y + (f.crop_y >> sh)) * f.pic_stride[c] + x + (f.crop_x >> sh);
                planes_out[o++] = pel == 1 ? tmp[idx] : reinterpret_cast<const uint16_t*>(tmp.data())[idx];
            }
    }
    return 0;
}

// the 8-bit planes K4 reads for one picture with output options o (h2j_engine_decode_scaled / _resized)
// (nrend renditions in flight, planes of rendition `pick`: h2j_engine_decode_multi)
// (info_n: entries of info the call has -- 4; 8: the window; 10: the orientation too; 12: qscale and sharpen too; 18: the
// padding too; 21: the colour too)
static int decode_jpeg_source(h2j_engine* w, const uint8_t* data, size_t size, const h2j_out_opts8* o, int nrend, int pick,
                              uint8_t* planes_out, size_t cap, int* info, int info_n = 4) {
    if (!w || !data || !planes_out || !info || !o) return -1;
    Engine& e = w->e;
    for (int r = 0; r < nrend; r++)
        if (!h2j::out_opts_valid(o[r])) {
            e.fail("invalid output options");
            return H2J_ERR_OUT_OPTS;
        }
    if (single_job(w, data, size, o, nrend)) return -2;
    for (int r = 0; r < nrend; r++)
        if (e.jobs[0].outs[r].error == H2J_ERR_NO_STAGE) {
            e.fail(h2j::no_stage_message(e.jobs[0].outs[r]));
            return H2J_ERR_NO_STAGE;
        } else if (e.jobs[0].outs[r].error) {  // a window outside the picture
            e.fail(h2j::out_opts_message(o[r], e.jobs[0].hdr.out_w, e.jobs[0].hdr.out_h, e.jobs[0].sei_orient, e.jobs[0].colour));
            return H2J_ERR_OUT_OPTS;
        }
    Slot& s = e.slot[0];
    // (12 entries: K4 runs too, for the quantiser scale it used)
    if (e.enqueue(s, info_n >= 12 ? 4 : 3, false) || e.sync(s)) return -3;
    // the picture K4 would read: the JPEG source view of the rendition
    const h2j_frame& f = s.plan.frames[0];
    const int vi = s.plan.rends[static_cast<size_t>(pick)].view;
    // (a padded rendition's view is its canvas; the mode is that of the view of its picture part)
    const bool padded = s.plan.vpad[vi] >= 0;
    const h2j_scaled& sc = s.plan.scaled[padded ? s.plan.padsrc[s.plan.vpad[vi]] : vi];
    const h2j_frame v = s.plan.view(vi);
    const int w_ = v.out_w, h_ = v.out_h;
    int levels = 0;  // K3s levels among the views of the same window: two or more are K3p's
    for (int x = 0; x < s.plan.nv; x++)
        if (s.plan.scaled[x].scale_log2 >= 1 && s.plan.scaled[x].scale_log2 <= 3 && s.plan.vsrc[x] == s.plan.vsrc[padded ? s.plan.padsrc[s.plan.vpad[vi]] : vi])
            levels |= 1 << s.plan.scaled[x].scale_log2;
    info[0] = w_;
    info[1] = h_;
    info[2] = (sc.scale_log2 >= 1 && sc.scale_log2 <= 3 && (levels & (levels - 1))) ? 5 : sc.scale_log2;
    info[3] = f.bit_depth;
    const h2j::FrameJob::Output& wo = e.jobs[0].outs[pick];
    if (info_n >= 8) {
        info[4] = wo.win_x;
        info[5] = wo.win_y;
        info[6] = wo.win_w;
        info[7] = wo.win_h;
    }
    if (info_n >= 10) {
        info[8] = wo.orient;
        info[9] = e.jobs[0].sei_orient;
    }
    if (info_n >= 12) {
        h2j_jstat st;
        if (h2j_gpu_memcpy_d2h(&st, static_cast<uint8_t*>(s.d_arena.p) + v.jstat, sizeof(st), s.stream) || h2j_gpu_stream_sync(s.stream))
            return e.fail(h2j_gpu_last_error());
        info[10] = st.qscale;
        info[11] = wo.sharpen;
    }
    if (info_n >= 18) {
        info[12] = wo.pad;
        info[13] = wo.pad_x;
        info[14] = wo.pad_y;
        info[15] = wo.out_w();
        info[16] = wo.out_h();
        info[17] = wo.fill[0] | (wo.fill[1] << 8) | (wo.fill[2] << 16);
    }
    if (info_n >= 21) {
        info[18] = wo.col_matrix;
        info[19] = wo.col_full;
        info[20] = wo.colour ? 1 : 0;
    }
    if (cap < static_cast<size_t>(w_) * h_ * 3 / 2) return e.fail("output buffer too small");
    const size_t pel = v.bit_depth > 8 ? 2 : 1;
    size_t bytes = 0;  // the view's planes in the arena, from v.pic2
    for (int c = 0; c < 3; c++) {
        // (an unscaled oriented view lies in the oriented planes, whose rows end with the oriented picture's)
        const int rows = (sc.scale_log2 || wo.sharpen || padded || wo.colour) ? (h_ >> (c ? 1 : 0)) : wo.orient ? ((v.crop_y + h_) >> (c ? 1 : 0)) : (f.height >> (c ? 1 : 0));
        bytes = std::max(bytes, (static_cast<size_t>(v.pic_off[c]) + static_cast<size_t>(v.pic_stride[c]) * rows) * pel);
    }
    std::vector<uint8_t> tmp(bytes);
    if (h2j_gpu_memcpy_d2h(tmp.data(), static_cast<uint8_t*>(s.d_arena.p) + v.pic2, bytes, s.stream) ||
        h2j_gpu_stream_sync(s.stream))
        return e.fail(h2j_gpu_last_error());
    size_t o_ = 0;
    for (int c = 0; c < 3; c++) {
        const int sh = c ? 1 : 0, bd = c ? v.bit_depth_c : v.bit_depth;
        for (int y = 0; y < (h_ >> sh); y++)
            for (int x = 0; x < (w_ >> sh); x++) {
                const size_t idx = static_cast<size_t>(v.pic_off[c]) +
                                   static_cast<size_t>(y + (v.crop_y >> sh)) * v.pic_stride[c] + x + (v.crop_x >> sh);
                int val = pel == 1 ? tmp[idx] : reinterpret_cast<const uint16_t*>(tmp.data())[idx];
                if (bd > 8) val = std::min(255, (val + (1 << (bd - 9))) >> (bd - 8));  // K4's conversion (jpeg_sample)
                planes_out[o_++] = static_cast<uint8_t>(val);
            }
    }
    return 0;
}

// info_n: the entries of info the call's option type has
template <typename T>
static int decode_multi_any(h2j_engine* w, const uint8_t* data, size_t size, int nrend, const T* opts, int pick, uint8_t* planes_out,
                            size_t cap, int* info, int info_n) {
    if (nrend < 1 || nrend > H2J_MAX_RENDITIONS) return H2J_ERR_RENDITIONS;
    if (pick < 0 || pick >= nrend || !opts) return -1;
    return decode_jpeg_source(w, data, size, h2j::to_opts8(nrend, opts).data(), nrend, pick, planes_out, cap, info, info_n);
}

// the engine calls of libH265ToJpegExt.so (api_ext.h): the multi6 calls with h2j_out_opts7 and h2j_out_opts8
namespace h2j {
int64_t submit_multi7(h2j_engine* w, int n, const uint8_t* const* data, const size_t* sizes, const int32_t* nrend, const h2j_out_opts7* opts,
                      uint8_t* out, size_t out_cap, size_t* out_off, size_t* out_len, int* status, int32_t* out_wh, bool latency) {
    return submit_multi_any(w, n, data, sizes, nrend, opts, out, out_cap, out_off, out_len, status, latency, out_wh);
}
int decode_multi7(h2j_engine* w, const uint8_t* data, size_t size, int nrend, const h2j_out_opts7* opts, int pick, uint8_t* planes_out,
                  size_t cap, int* info) {
    return decode_multi_any(w, data, size, nrend, opts, pick, planes_out, cap, info, 18);
}
int64_t submit_multi8(h2j_engine* w, int n, const uint8_t* const* data, const size_t* sizes, const int32_t* nrend, const h2j_out_opts8* opts,
                      uint8_t* out, size_t out_cap, size_t* out_off, size_t* out_len, int* status, int32_t* out_wh, bool latency) {
    return submit_multi_any(w, n, data, sizes, nrend, opts, out, out_cap, out_off, out_len, status, latency, out_wh);
}
int decode_multi8(h2j_engine* w, const uint8_t* data, size_t size, int nrend, const h2j_out_opts8* opts, int pick, uint8_t* planes_out,
                  size_t cap, int* info) {
    return decode_multi_any(w, data, size, nrend, opts, pick, planes_out, cap, info, 21);
}
int stream_colour(const uint8_t* data, size_t size, int32_t* info) {
    if (!data || !info) return -1;
    int c[4] = {2, 2, 2, 0};
    int rc = 0;
    if (is_heif(data, size)) {
        rc = heif_stream_colour(data, size, c);
    } else {
        const int codec = detect_codec(data, size);
        if (codec != 264 && codec != 265) return -100;
        // (a stream without an SPS that parses signals nothing)
        if (codec == 265) hevc_stream_colour(data, size, c);
        else h264_stream_colour(data, size, c);
    }
    if (rc) return rc;
    for (int i = 0; i < 4; i++) info[i] = c[i];
    return 0;
}
}  // namespace h2j

extern "C" {

const char* h2j_version(void) { return "h2j-mi355x 0.2 (gfx950, HIP)"; }

h2j_engine* h2j_engine_create(int device, int host_threads) {
    if (h2j_gpu_device_count() <= 0) return nullptr;
    if (h2j_gpu_set_device(device) != 0) return nullptr;
    h2j_engine* w = new h2j_engine();
    Engine& e = w->e;
    e.device = device;
    for (auto& s : e.slot) {
        s.stream = h2j_gpu_stream_create();
        if (!s.stream) {
            delete w;
            return nullptr;
        }
        for (auto& ev : s.ev) ev = h2j_gpu_event_create();
    }
    // host pool: NUMA-local to the device, sized by the CPU mask / cgroup quota (affinity.h)
    std::vector<int> nodes;
    const int ndev = h2j_gpu_device_count();
    for (int i = 0; i < ndev; i++) {
        char bus[64] = {0};
        nodes.push_back(h2j_gpu_pci_bus_id(i, bus, sizeof(bus)) == 0 ? h2j::pci_numa_node(bus) : -1);
    }
    const int node = device >= 0 && device < ndev ? nodes[device] : -1;
    e.plan = h2j::plan_host(device, nodes, h2j::process_cpus(), h2j::node_cpus(node), h2j::cgroup_cpu_quota(),
                            host_threads > 0 ? host_threads : 0, host_threads < 0 ? -host_threads : 1);
    e.pool = new h2j::ThreadPool(e.plan.threads - 1, e.plan.cpus);
    // HBM per slot: 64 GB at most, and the device's memory split between the two slots of every
    // engine of this process on the device (host_threads = -k: k engines dealt over the devices)
    const int k = host_threads < 0 ? -host_threads : 1;
    const int per_dev = std::max(1, k / std::max(1, ndev) + (device < k % std::max(1, ndev) ? 1 : 0));
    size_t free_b = 0, total_b = 0;
    double budget = h2j::kSlotHbmBudget;
    if (h2j_gpu_mem_info(&free_b, &total_b) == 0 && total_b > 0)
        budget = std::min(budget, 0.8 * static_cast<double>(total_b) / (2.0 * per_dev));
    e.slot_hbm_budget = budget;
    const char* strict = std::getenv("H2J_STRICT_REFERENCE");
    e.strict_reference = strict && strict[0] == '1';
    return w;
}

void h2j_engine_destroy(h2j_engine* e) { delete e; }

const char* h2j_engine_error(h2j_engine* e) { return e ? e->e.err.c_str() : "no engine"; }

int64_t h2j_engine_submit(h2j_engine* w, int n, const uint8_t* const* data, const size_t* sizes, uint8_t* out,
                          size_t out_cap, size_t* out_off, size_t* out_len, int* status) {
    if (!w || n < 0) return -1;
    return submit_batch(w, n, data, sizes, nullptr, nullptr, out, out_cap, out_off, out_len, status, false);
}

int64_t h2j_engine_submit_opts(h2j_engine* w, int n, const uint8_t* const* data, const size_t* sizes,
                               const h2j_out_opts* opts, uint8_t* out, size_t out_cap, size_t* out_off, size_t* out_len,
                               int* status) {
    if (!w || n < 0) return -1;
    return submit_batch(w, n, data, sizes, nullptr, h2j::to_opts8(n, opts).data(), out, out_cap, out_off, out_len, status, false);
}

int64_t h2j_engine_submit_opts2(h2j_engine* w, int n, const uint8_t* const* data, const size_t* sizes,
                                const h2j_out_opts2* opts, uint8_t* out, size_t out_cap, size_t* out_off,
                                size_t* out_len, int* status) {
    if (!w || n < 0) return -1;
    return submit_batch(w, n, data, sizes, nullptr, h2j::to_opts8(n, opts).data(), out, out_cap, out_off, out_len, status, false);
}

int h2j_engine_wait(h2j_engine* w, int64_t ticket) {
    if (!w) return -1;
    Engine& e = w->e;
    std::unique_lock<std::mutex> lk(e.amu);
    auto it = std::find_if(e.batches.begin(), e.batches.end(),
                           [&](const std::unique_ptr<h2j::Batch>& b) { return b->ticket == ticket; });
    if (it == e.batches.end()) return -1;
    h2j::Batch* b = it->get();
    e.acv.wait(lk, [&] { return b->done; });
    const int rc = b->rc;
    std::memcpy(e.last_stats, b->stats, sizeof(b->stats));
    e.last_chunk_log.swap(b->chunk_log);
    e.last_status.assign(b->status, b->status + b->nout);
    e.last_msg.swap(b->msg);
    if (rc) e.err = b->err;
    e.batches.erase(it);
    return rc;
}

int h2j_engine_transcode(h2j_engine* w, int n, const uint8_t* const* data, const size_t* sizes, uint8_t* out,
                         size_t out_cap, size_t* out_off, size_t* out_len, int* status) {
    if (!w) return -1;
    const int64_t t = submit_batch(w, n, data, sizes, nullptr, nullptr, out, out_cap, out_off, out_len, status, true);
    return h2j_engine_wait(w, t);
}

int h2j_engine_transcode_opts(h2j_engine* w, int n, const uint8_t* const* data, const size_t* sizes,
                              const h2j_out_opts* opts, uint8_t* out, size_t out_cap, size_t* out_off, size_t* out_len,
                              int* status) {
    if (!w || n < 0) return -1;
    const int64_t t = submit_batch(w, n, data, sizes, nullptr, h2j::to_opts8(n, opts).data(), out, out_cap, out_off, out_len, status, true);
    return h2j_engine_wait(w, t);
}

int h2j_engine_transcode_opts2(h2j_engine* w, int n, const uint8_t* const* data, const size_t* sizes,
                               const h2j_out_opts2* opts, uint8_t* out, size_t out_cap, size_t* out_off,
                               size_t* out_len, int* status) {
    if (!w || n < 0) return -1;
    const int64_t t = submit_batch(w, n, data, sizes, nullptr, h2j::to_opts8(n, opts).data(), out, out_cap, out_off, out_len, status, true);
    return h2j_engine_wait(w, t);
}

int64_t h2j_engine_submit_multi(h2j_engine* w, int n, const uint8_t* const* data, const size_t* sizes, const int32_t* nrend, const h2j_out_opts2* opts,
                                uint8_t* out, size_t out_cap, size_t* out_off, size_t* out_len, int* status) {
    return submit_multi_any(w, n, data, sizes, nrend, opts, out, out_cap, out_off, out_len, status, false);
}
int64_t h2j_engine_submit_multi3(h2j_engine* w, int n, const uint8_t* const* data, const size_t* sizes, const int32_t* nrend, const h2j_out_opts3* opts,
                                 uint8_t* out, size_t out_cap, size_t* out_off, size_t* out_len, int* status) {
    return submit_multi_any(w, n, data, sizes, nrend, opts, out, out_cap, out_off, out_len, status, false);
}
int64_t h2j_engine_submit_multi4(h2j_engine* w, int n, const uint8_t* const* data, const size_t* sizes, const int32_t* nrend, const h2j_out_opts4* opts,
                                 uint8_t* out, size_t out_cap, size_t* out_off, size_t* out_len, int* status) {
    return submit_multi_any(w, n, data, sizes, nrend, opts, out, out_cap, out_off, out_len, status, false);
}
int64_t h2j_engine_submit_multi5(h2j_engine* w, int n, const uint8_t* const* data, const size_t* sizes, const int32_t* nrend, const h2j_out_opts5* opts,
                                 uint8_t* out, size_t out_cap, size_t* out_off, size_t* out_len, int* status) {
    return submit_multi_any(w, n, data, sizes, nrend, opts, out, out_cap, out_off, out_len, status, false);
}
int64_t h2j_engine_submit_multi6(h2j_engine* w, int n, const uint8_t* const* data, const size_t* sizes, const int32_t* nrend, const h2j_out_opts6* opts,
                                 uint8_t* out, size_t out_cap, size_t* out_off, size_t* out_len, int* status, int32_t* out_wh) {
    return submit_multi_any(w, n, data, sizes, nrend, opts, out, out_cap, out_off, out_len, status, false, out_wh);
}
int h2j_engine_transcode_multi(h2j_engine* w, int n, const uint8_t* const* data, const size_t* sizes, const int32_t* nrend, const h2j_out_opts2* opts,
                               uint8_t* out, size_t out_cap, size_t* out_off, size_t* out_len, int* status) {
    return static_cast<int>(submit_multi_any(w, n, data, sizes, nrend, opts, out, out_cap, out_off, out_len, status, true));
}
int h2j_engine_transcode_multi3(h2j_engine* w, int n, const uint8_t* const* data, const size_t* sizes, const int32_t* nrend, const h2j_out_opts3* opts,
                                uint8_t* out, size_t out_cap, size_t* out_off, size_t* out_len, int* status) {
    return static_cast<int>(submit_multi_any(w, n, data, sizes, nrend, opts, out, out_cap, out_off, out_len, status, true));
}
int h2j_engine_transcode_multi4(h2j_engine* w, int n, const uint8_t* const* data, const size_t* sizes, const int32_t* nrend, const h2j_out_opts4* opts,
                                uint8_t* out, size_t out_cap, size_t* out_off, size_t* out_len, int* status) {
    return static_cast<int>(submit_multi_any(w, n, data, sizes, nrend, opts, out, out_cap, out_off, out_len, status, true));
}
int h2j_engine_transcode_multi5(h2j_engine* w, int n, const uint8_t* const* data, const size_t* sizes, const int32_t* nrend, const h2j_out_opts5* opts,
                                uint8_t* out, size_t out_cap, size_t* out_off, size_t* out_len, int* status) {
    return static_cast<int>(submit_multi_any(w, n, data, sizes, nrend, opts, out, out_cap, out_off, out_len, status, true));
}
int h2j_engine_transcode_multi6(h2j_engine* w, int n, const uint8_t* const* data, const size_t* sizes, const int32_t* nrend, const h2j_out_opts6* opts,
                                uint8_t* out, size_t out_cap, size_t* out_off, size_t* out_len, int* status, int32_t* out_wh) {
    return static_cast<int>(submit_multi_any(w, n, data, sizes, nrend, opts, out, out_cap, out_off, out_len, status, true, out_wh));
}

int h2j_fit_size(int w, int h, int fit_w, int fit_h, int flags, int* ow, int* oh) { return h2j::fit_size(w, h, fit_w, fit_h, flags, ow, oh); }
int h2j_crop_window(int w, int h, const h2j_out_opts3* o, int32_t* win, int* ow, int* oh) {
    int orient = 0;
    return h2j::crop_window(w, h, o, 0, win, ow, oh, &orient);
}
int h2j_crop_window4(int w, int h, const h2j_out_opts4* o, int sei_orient, int32_t* win, int* ow, int* oh, int* orient) {
    return h2j::crop_window(w, h, o, sei_orient, win, ow, oh, orient);
}
int h2j_crop_window5(int w, int h, const h2j_out_opts5* o, int sei_orient, int32_t* win, int* ow, int* oh, int* orient) {
    return h2j::crop_window(w, h, o, sei_orient, win, ow, oh, orient);
}
int h2j_crop_window6(int w, int h, const h2j_out_opts6* o, int sei_orient, int32_t* win, int* ow, int* oh, int* orient) {
    return h2j::crop_window(w, h, o, sei_orient, win, ow, oh, orient);
}

int h2j_stream_orientation(const uint8_t* data, size_t size) {
    if (!data) return -1;
    if (h2j::is_heif(data, size)) return h2j::heif_orientation(data, size);
    const int codec = h2j::detect_codec(data, size);
    if (codec != 264 && codec != 265) return -100;
    return h2j::stream_display_orientation(data, size, codec);
}

int h2j_engine_decode(h2j_engine* w, const uint8_t* data, size_t size, int stage, uint16_t* planes_out,
                      size_t cap, int* info) {
    if (!w) return -1;
    Engine& e = w->e;
    if (single_job(w, data, size)) return -2;
    const int stages = stage == 1 ? 1 : (stage == 2 ? 2 : 3);
    Slot& s = e.slot[0];
    if (e.enqueue(s, stages, false) || e.sync(s)) return -3;
    return copy_planes(e, s, 0, stage, planes_out, cap, info);
}

int h2j_engine_decode_batch(h2j_engine* w, int n, const uint8_t* const* data, const size_t* sizes, int stage, int pick,
                            uint16_t* planes_out, size_t cap, int* info) {
    if (!w || n <= 0 || pick < 0 || pick >= n) return -1;
    Engine& e = w->e;
    e.quiesce();
    if (h2j_gpu_set_device(e.device)) return e.fail(h2j_gpu_last_error());
    e.jobs.resize(n);
    std::vector<int> rc(n, 0);
    e.par(n, [&](int i) {
        e.jobs[i].threads = 1;
        rc[i] = h2j::parse_any(data[i], sizes[i], e.jobs[i]);
        if (rc[i] == 0) h2j::resolve_outputs(&h2j::kPlainOutput8, 1, e.jobs[i]);
    });
    for (int i = 0; i < n; i++)
        if (rc[i]) {
            e.fail("parse failed (picture " + std::to_string(i) + "): " + e.jobs[i].message);
            return -2;
        }
    Slot& s = e.slot[0];
    s.live.resize(n);
    for (int i = 0; i < n; i++) s.live[i] = i;
    s.jobs = &e.jobs;
    const int stages = stage == 1 ? 1 : (stage == 2 ? 2 : 3);
    if (e.enqueue(s, stages, false) || e.sync(s)) return -3;
    return copy_planes(e, s, pick, stage, planes_out, cap, info);
}

int h2j_engine_jpeg_coeffs(h2j_engine* w, const uint8_t* data, size_t size, int16_t* out, size_t cap, int* info) {
    if (!w) return -1;
    Engine& e = w->e;
    if (single_job(w, data, size)) return -2;
    Slot& s = e.slot[0];
    if (e.enqueue(s, 4, false) || e.sync(s)) return -3;
    const h2j_frame& f = s.plan.frames[0];
    const int nmcu = ((f.out_w + 15) >> 4) * ((f.out_h + 15) >> 4);
    h2j_jstat st;
    if (cap < static_cast<size_t>(nmcu) * 384) return e.fail("output buffer too small");
    if (h2j_gpu_memcpy_d2h(&st, static_cast<uint8_t*>(s.d_arena.p) + f.jstat, sizeof(st), s.stream) ||
        h2j_gpu_memcpy_d2h(out, static_cast<uint8_t*>(s.d_arena.p) + f.jcoef, static_cast<size_t>(nmcu) * 384 * 2,
                           s.stream) ||
        h2j_gpu_stream_sync(s.stream))
        return e.fail(h2j_gpu_last_error());
    info[0] = f.out_w;
    info[1] = f.out_h;
    info[2] = st.qscale;
    info[3] = nmcu;
    return 0;
}

int h2j_engine_decode_scaled(h2j_engine* w, const uint8_t* data, size_t size, int scale_log2, int max_dim,
                             uint8_t* planes_out, size_t cap, int* info) {
    const h2j_out_opts8 o = {scale_log2, max_dim, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    return decode_jpeg_source(w, data, size, &o, 1, 0, planes_out, cap, info);
}

int h2j_engine_decode_resized(h2j_engine* w, const uint8_t* data, size_t size, int fit_w, int fit_h, int flags,
                              uint8_t* planes_out, size_t cap, int* info) {
    const h2j_out_opts8 o = {0, 0, fit_w, fit_h, flags, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    return decode_jpeg_source(w, data, size, &o, 1, 0, planes_out, cap, info);
}

int h2j_engine_decode_multi(h2j_engine* w, const uint8_t* data, size_t size, int nrend, const h2j_out_opts2* opts, int pick,
                            uint8_t* planes_out, size_t cap, int* info) {
    return decode_multi_any(w, data, size, nrend, opts, pick, planes_out, cap, info, 4);
}
int h2j_engine_decode_multi3(h2j_engine* w, const uint8_t* data, size_t size, int nrend, const h2j_out_opts3* opts, int pick,
                             uint8_t* planes_out, size_t cap, int* info) {
    return decode_multi_any(w, data, size, nrend, opts, pick, planes_out, cap, info, 8);
}
int h2j_engine_decode_multi4(h2j_engine* w, const uint8_t* data, size_t size, int nrend, const h2j_out_opts4* opts, int pick,
                             uint8_t* planes_out, size_t cap, int* info) {
    return decode_multi_any(w, data, size, nrend, opts, pick, planes_out, cap, info, 10);
}
int h2j_engine_decode_multi5(h2j_engine* w, const uint8_t* data, size_t size, int nrend, const h2j_out_opts5* opts, int pick,
                             uint8_t* planes_out, size_t cap, int* info) {
    return decode_multi_any(w, data, size, nrend, opts, pick, planes_out, cap, info, 12);
}

int h2j_engine_host_info(h2j_engine* w, int* out, int n) {
    if (!w) return -1;
    const Engine& e = w->e;
    const int v[4] = {e.pool->size() + 1, e.plan.numa_node, e.pool->pinned() ? static_cast<int>(e.plan.cpus.size()) : 0,
                      e.plan.cpus.empty() ? -1 : e.plan.cpus[0]};
    for (int i = 0; i < n && i < 4; i++) out[i] = v[i];
    return 0;
}

const char* h2j_engine_frame_error(h2j_engine* w, int i) {
    if (!w) return "";
    std::lock_guard<std::mutex> g(w->e.amu);
    if (i < 0 || i >= static_cast<int>(w->e.last_status.size())) return "";
    switch (w->e.last_status[i]) {
    case 0: return "";
    case -50: return "output buffer too small";
    case -51: return "JPEG payload pool overflow";
    case -52: return "device-side failure (a K1 / deblocking progress wait timed out)";
    default: {
        // copied under the lock into a per-thread buffer: h2j_engine_wait on another thread may
        // replace last_msg (and free its strings) as soon as the lock is released
        static thread_local std::string buf;
        buf = i < static_cast<int>(w->e.last_msg.size()) ? w->e.last_msg[i] : std::string();
        return buf.c_str();
    }
    }
}

int h2j_device_count(void) { return h2j_gpu_device_count(); }

int h2j_engine_chunk_times(h2j_engine* w, double* out, int max_chunks) {
    if (!w) return -1;
    std::lock_guard<std::mutex> g(w->e.amu);
    const auto& log = w->e.last_chunk_log;
    const int n = static_cast<int>(log.size());
    for (int i = 0; i < n && i < max_chunks; i++) {
        out[3 * i] = log[i].frames;
        out[3 * i + 1] = log[i].k1_ms;
        out[3 * i + 2] = log[i].kernels_ms;
    }
    return n;
}

int h2j_engine_stats(h2j_engine* w, double* out, int n) {
    if (!w) return -1;
    std::lock_guard<std::mutex> g(w->e.amu);
    for (int i = 0; i < n && i < h2j::ST_N; i++) out[i] = w->e.last_stats[i];
    return 0;
}

}  // extern "C"
