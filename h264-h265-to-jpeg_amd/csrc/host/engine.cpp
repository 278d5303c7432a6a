// Batch engine: host entropy threads -> HBM job records -> HIP pixel and
// JPEG pipeline -> host container assembly.  One engine per process per GPU;
// the IDecoder facade and the C ABI (include/h2j.h) both run on it.
//
// A batch is cut into chunks that flow through two slots (HIP stream +
// device/pinned buffers each), so the host parses chunk c+1 and assembles
// chunk c-1 while the GPU runs chunk c.  Per chunk:
//   1. parse      — pool threads run the H.264/H.265 entropy decoders
//                   (hevc_parser.cpp / h264_parser.cpp) into FrameJobs
//   2. pack + H2D — job records packed into one pinned staging buffer, one copy
//   3. GPU        — K1 recon, K2 deblock, K3 SAO, K4 JPEG forward path,
//                   K5 Huffman tables + entropy-coded payload
//   4. D2H        — per-frame tables (h2j_jstat) and the packed payloads only
//   5. assemble   — pool threads write the JPEG containers (jpeg_writer.cpp)
// This is what the reference does per call inside FFmpeg between
// avcodec_send_packet (/root/reference/src/Decoder.cpp:324) and
// av_write_frame (/root/reference/src/Encoder.cpp:278).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <deque>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include <pthread.h>
#include <sched.h>

#include "affinity.h"
#include "bitstream.h"
#include "chunk_plan.h"
#include "h2j.h"
#include "h2j_gpu.h"
#include "job.h"
#include "jpeg_writer.h"

// the kernel library's orientation stage, null when the library in use is older than it (a weak reference:
// bound when this library loads, so a stand-in or an older build selected beside it still loads)
extern "C" int h2j_gpu_orient(const h2j_gpu_batch*, const h2j_orient*, const int32_t*, const int32_t*, const int32_t*, void*)
    __attribute__((weak));
// likewise its finishing stage: K3u and the K4 entry that takes the quantiser scale from the caller
extern "C" int h2j_gpu_finish(const h2j_gpu_batch*, const h2j_finish*, const int32_t*, const int32_t*, const int32_t*, void*)
    __attribute__((weak));
extern "C" int h2j_gpu_jpeg2(const h2j_gpu_batch*, const int32_t*, void*) __attribute__((weak));
// likewise its RGB stage: K3c
extern "C" int h2j_gpu_rgb(const h2j_gpu_batch*, const h2j_rgb*, const int32_t*, const int32_t*, const int32_t*, void*)
    __attribute__((weak));

namespace h2j {
namespace {

double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

class ThreadPool {
public:
    // n workers; cpus: if non-empty, every worker runs on that CPU set (NUMA-local slice)
    explicit ThreadPool(int n, const std::vector<int>& cpus = std::vector<int>()) : stop_(false), gen_(0), pending_(0) {
        for (int i = 0; i < n; i++) workers_.emplace_back([this] { loop(); });
        if (!cpus.empty()) {
            cpu_set_t set;
            CPU_ZERO(&set);
            for (int c : cpus)
                if (c >= 0 && c < CPU_SETSIZE) CPU_SET(c, &set);
            for (auto& t : workers_)
                if (pthread_setaffinity_np(t.native_handle(), sizeof(set), &set) == 0) pinned_ = true;
        }
    }
    bool pinned() const { return pinned_; }
    ~ThreadPool() {
        {
            std::lock_guard<std::mutex> g(m_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto& t : workers_) t.join();
    }
    int size() const { return static_cast<int>(workers_.size()); }
    // run f(i) for i in [0, n) on the pool (caller participates)
    void parallel_for(int n, const std::function<void(int)>& f) {
        if (n <= 0) return;
        if (workers_.empty() || n == 1) {
            for (int i = 0; i < n; i++) f(i);
            return;
        }
        std::atomic<int> next(0);
        auto body = [&]() {
            for (;;) {
                int i = next.fetch_add(1);
                if (i >= n) break;
                f(i);
            }
        };
        {
            std::lock_guard<std::mutex> g(m_);
            task_ = body;
            pending_ = static_cast<int>(workers_.size());
            gen_++;
        }
        cv_.notify_all();
        body();
        std::unique_lock<std::mutex> lk(m_);
        done_.wait(lk, [this] { return pending_ == 0; });
        task_ = nullptr;
    }

private:
    void loop() {
        unsigned long seen = 0;
        for (;;) {
            std::function<void()> t;
            {
                std::unique_lock<std::mutex> lk(m_);
                cv_.wait(lk, [&] { return stop_ || gen_ != seen; });
                if (stop_) return;
                seen = gen_;
                t = task_;
            }
            if (t) t();
            {
                std::lock_guard<std::mutex> g(m_);
                if (--pending_ == 0) done_.notify_all();
            }
        }
    }
    std::vector<std::thread> workers_;
    std::mutex m_;
    std::condition_variable cv_, done_;
    std::function<void()> task_;
    bool pinned_ = false;
    bool stop_;
    unsigned long gen_;
    int pending_;
};

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    bool ensure(size_t n) {
        if (n <= cap) return true;
        if (p) h2j_gpu_free(p);
        cap = std::max(n, cap + cap / 2);
        p = h2j_gpu_malloc(cap);
        if (!p) cap = 0;
        return p != nullptr;
    }
    void release() {
        if (p) h2j_gpu_free(p);
        p = nullptr;
        cap = 0;
    }
};

struct HostBuf {
    uint8_t* p = nullptr;
    size_t cap = 0;
    bool ensure(size_t n) {
        if (n <= cap) return true;
        if (p) h2j_gpu_host_free(p);
        cap = std::max(n, cap + cap / 2);
        p = static_cast<uint8_t*>(h2j_gpu_host_alloc(cap));
        if (!p) cap = 0;
        return p != nullptr;
    }
    void release() {
        if (p) h2j_gpu_host_free(p);
        p = nullptr;
        cap = 0;
    }
};

int parse_any(const uint8_t* d, size_t n, FrameJob& job) {
    const int codec = detect_codec(d, n);
    if (codec == 265) return hevc_parse_picture(d, n, job);
    if (codec == 264) return h264_parse_picture(d, n, job);
    job.clear();
    job.error = -100;
    job.message = "not an H.264/H.265 Annex-B stream";
    return -100;
}

// Output options: h2j_out_opts6 is the engine's one option type (an h2j_out_opts item has the fit fields 0,
// an h2j_out_opts2 item the crop fields, an h2j_out_opts3 item the orientation, an h2j_out_opts4 item qscale and
// sharpen, an h2j_out_opts5 item the format: widen_opts4, widen_opts5 in job.h)
const h2j_out_opts6 kPlainOutput = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, {0, 0, 0}};  // the JPEG at the decoded size
std::vector<h2j_out_opts6> opts6_of(int n, const h2j_out_opts* o) {  // o null: all plain
    std::vector<h2j_out_opts6> v(static_cast<size_t>(std::max(n, 0)), kPlainOutput);
    for (int i = 0; o && i < n; i++) {
        v[i].scale_log2 = o[i].scale_log2;
        v[i].max_dim = o[i].max_dim;
    }
    return v;
}
h2j_out_opts6 opts6_of(const h2j_out_opts5& o) { return widen_opts5(o); }
h2j_out_opts6 opts6_of(const h2j_out_opts4& o) { return widen_opts5(widen_opts4(o)); }
h2j_out_opts6 opts6_of(const h2j_out_opts3& o) {
    return h2j_out_opts6{o.scale_log2, o.max_dim, o.fit_w, o.fit_h, o.flags, o.crop_x, o.crop_y, o.crop_w, o.crop_h, 0, 0, 0, 0,
                         {o.reserved[0], o.reserved[1], o.reserved[2]}};
}
h2j_out_opts6 opts6_of(const h2j_out_opts2& o) {
    return h2j_out_opts6{o.scale_log2, o.max_dim, o.fit_w, o.fit_h, o.flags, 0, 0, 0, 0, 0, 0, 0, 0, {o.reserved[0], o.reserved[1], o.reserved[2]}};
}
template <typename T>
std::vector<h2j_out_opts6> opts6_of(int n, const T* o) {  // h2j_out_opts2 / h2j_out_opts3 items
    std::vector<h2j_out_opts6> v(static_cast<size_t>(std::max(n, 0)), kPlainOutput);
    for (int i = 0; o && i < n; i++) v[i] = opts6_of(o[i]);
    return v;
}
// the h2j_out_opts6 items of a multi call's h2j_out_opts2 / h2j_out_opts3 items (valid counts)
template <typename T>
std::vector<h2j_out_opts6> multi_opts6(int n, const int32_t* nrend, const T* opts) {
    int total = 0;
    for (int i = 0; i < n; i++) total += nrend[i];
    return opts6_of(total, opts);
}
bool reserved_zero(const h2j_out_opts6& o) { return std::all_of(o.reserved, o.reserved + 3, [](int32_t r) { return r == 0; }); }
// finishing (include/h2j.h "Finishing"): a fixed quantiser scale, an unsharp mask
bool finish_valid(const h2j_out_opts6& o) { return (o.qscale == 0 || (o.qscale >= 2 && o.qscale <= 31)) && o.sharpen >= 0 && o.sharpen <= 64; }
bool finishing(const FrameJob::Output& o) { return o.qscale != 0 || o.sharpen != 0; }
// RGB output (include/h2j.h "RGB output"): a known format, and no quantiser scale for pixels
bool format_valid(const h2j_out_opts6& o) { return o.format >= H2J_FMT_JPEG && o.format <= H2J_FMT_RGB8_PLANAR && !(o.format && o.qscale); }
// the orientation (0, 2..8) the options name for a picture whose display orientation SEI says sei_orient
int resolve_orient(const h2j_out_opts6& o, int sei_orient) {
    const int r = o.orient == H2J_ORIENT_AUTO ? sei_orient : o.orient;
    return r == 1 ? 0 : r;
}
const char kNoStageMessage[] = "the kernel library has no orientation stage (h2j_gpu_orient): oriented output needs a newer libh2j_hip.so";
const char kNoRgbMessage[] = "the kernel library has no RGB stage (h2j_gpu_rgb): raw output needs a newer libh2j_hip.so";
const char kNoFinishMessage[] = "the kernel library has no finishing stage (h2j_gpu_finish, h2j_gpu_jpeg2): qscale and sharpen need a newer libh2j_hip.so";
// Scaled output (include/h2j.h h2j_out_opts): the scale of a w x h picture -- scale_log2, or with
// max_dim > 0 the smallest k from scale_log2 up whose JPEG fits max_dim (3 if none does).
// Exact-size output (h2j_out_opts2): the size h2j_fit_size gives.
bool fit_valid(int fit_w, int fit_h, int flags) {
    return (fit_w == 0 || (fit_w >= 2 && fit_w <= 65535)) && (fit_h == 0 || (fit_h >= 2 && fit_h <= 65535)) &&
           (flags & ~H2J_FIT_STRETCH) == 0 && !((flags & H2J_FIT_STRETCH) && fit_w == 0 && fit_h == 0);
}
// what can be said of the options before the picture's size is known (an item none of whose renditions
// passes is not parsed); the window's place in the picture is checked by resolve_output
bool out_opts_valid(const h2j_out_opts6& o) {
    if (o.scale_log2 < 0 || o.scale_log2 > 3 || o.max_dim < 0) return false;
    if (!reserved_zero(o) || o.orient < H2J_ORIENT_AUTO || o.orient > 8 || !finish_valid(o) || !format_valid(o)) return false;
    if (o.crop_x < 0 || o.crop_y < 0 || o.crop_w < 0 || o.crop_h < 0 || ((o.crop_x | o.crop_y | o.crop_w | o.crop_h) & 1)) return false;
    if (o.flags & H2J_FIT_COVER) {  // a box, and nothing else that sizes the output
        if (o.flags != H2J_FIT_COVER || o.fit_w < 2 || o.fit_h < 2 || o.scale_log2 || o.max_dim) return false;
        return fit_valid(o.fit_w, o.fit_h, 0);
    }
    if (!fit_valid(o.fit_w, o.fit_h, o.flags)) return false;
    return !((o.fit_w || o.fit_h) && (o.scale_log2 || o.max_dim));
}
int resolve_scale(const h2j_out_opts6& o, int w, int h) {
    int k = o.scale_log2;
    if (o.max_dim > 0)
        while (k < 3 && std::max(h2j_scaled_dim(w, k), h2j_scaled_dim(h, k)) > o.max_dim) k++;
    return k;
}
// the output of a W x H picture (its parsed, cropped size) with options that passed out_opts_valid: the
// window (include/h2j.h "Crop and cover"; error H2J_ERR_OUT_OPTS if it does not lie in the picture), then
// what the remaining options make of a picture of the window's size.  A fit that resolves to the window's own
// size is the unscaled output; one that K3s makes on all three planes (w = ow 2^k, h = oh 2^k: the
// resampler's arithmetic reduces to K3s's there) is the scaled output of that k; K3r gets the rest.
// Orientation (include/h2j.h "Orientation"; sei_orient: the picture's, for H2J_ORIENT_AUTO) comes first: the
// rule runs on the oriented size, the window is in the oriented picture
FrameJob::Output resolve_output(const h2j_out_opts6& o, int W, int H, int sei_orient) {
    FrameJob::Output out;
    out.qscale = o.qscale;
    out.sharpen = o.sharpen;
    out.format = o.format;
    out.orient = resolve_orient(o, sei_orient);
    if (out.orient >= 5) std::swap(W, H);
    int64_t x = o.crop_x, y = o.crop_y, w = o.crop_w ? o.crop_w : W - x, h = o.crop_h ? o.crop_h : H - y;
    if (w < 2 || h < 2 || x + w > W || y + h > H) {
        out.error = H2J_ERR_OUT_OPTS;
        return out;
    }
    int fit_w = o.fit_w, fit_h = o.fit_h, flags = o.flags;
    if (flags & H2J_FIT_COVER) {  // the largest centred part of the window with the box's aspect, then a stretch
        const int64_t bw = fit_w, bh = fit_h;
        int64_t cw = w, ch = h;
        if (w * bh >= h * bw) cw = std::min(std::max<int64_t>(2 * ((h * bw) / (2 * bh)), 2), w);
        else ch = std::min(std::max<int64_t>(2 * ((w * bh) / (2 * bw)), 2), h);
        x += 2 * ((w - cw) / 4);
        y += 2 * ((h - ch) / 4);
        w = cw;
        h = ch;
        flags = H2J_FIT_STRETCH;
    }
    out.win_x = static_cast<int>(x);
    out.win_y = static_cast<int>(y);
    out.win_w = static_cast<int>(w);
    out.win_h = static_cast<int>(h);
    out.windowed = !(x == 0 && y == 0 && w == W && h == H);
    out.scale_log2 = resolve_scale(o, out.win_w, out.win_h);
    int ow = out.win_w, oh = out.win_h;
    if ((fit_w == 0 && fit_h == 0) || h2j_fit_size(out.win_w, out.win_h, fit_w, fit_h, flags, &ow, &oh) != 0) return out;
    if (ow == out.win_w && oh == out.win_h) return out;
    for (int k = 1; k <= 3; k++)
        if ((ow << k) == out.win_w && (oh << k) == out.win_h) {
            out.scale_log2 = k;
            return out;
        }
    out.scale_log2 = H2J_SCALE_RESAMPLE;
    out.fit_w = ow;
    out.fit_h = oh;
    return out;
}
// W, H: the parsed picture's cropped size (0: not parsed).  Options without a window or cover get the
// message they always got
std::string out_opts_message(const h2j_out_opts6& o, int W = 0, int H = 0, int sei_orient = 0) {
    std::string m = "invalid output options: scale_log2 " + std::to_string(o.scale_log2) + " (0..3), max_dim " +
           std::to_string(o.max_dim) + " (>= 0), fit " + std::to_string(o.fit_w) + " x " + std::to_string(o.fit_h) +
           " (0 or 2..65535, not with scale_log2 / max_dim), flags " + std::to_string(o.flags) +
           " (stretch needs a size), reserved " + (reserved_zero(o) ? "0" : "non-zero");
    const bool window = o.crop_x || o.crop_y || o.crop_w || o.crop_h || (o.flags & H2J_FIT_COVER);
    if (window)
        m += "; crop " + std::to_string(o.crop_x) + ", " + std::to_string(o.crop_y) + ", " + std::to_string(o.crop_w) + " x " +
             std::to_string(o.crop_h) + " (even, >= 0, at least 2 x 2 inside the picture; cover needs a box and excludes stretch, scale_log2, max_dim)";
    if (o.orient != 0) m += "; orient " + std::to_string(o.orient) + " (0..8, -1: the stream's display orientation)";
    if (o.qscale != 0 || o.sharpen != 0)
        m += "; qscale " + std::to_string(o.qscale) + " (0 or 2..31), sharpen " + std::to_string(o.sharpen) + " (0..64)";
    if (o.format != 0) m += "; format " + std::to_string(o.format) + " (0 JPEG, 1 RGB, 2 planar RGB; not with qscale)";
    if (!(window && W > 0 && H > 0)) return m;
    const int ro = (o.orient >= H2J_ORIENT_AUTO && o.orient <= 8) ? resolve_orient(o, sei_orient) : 0;
    if (ro >= 5) std::swap(W, H);
    m += "; the picture is " + std::to_string(W) + " x " + std::to_string(H);
    if (ro) m += " at orientation " + std::to_string(ro);
    return m;
}
// the message of an output that failed with H2J_ERR_NO_STAGE: the stage the kernel library lacks
const char* no_stage_message(const FrameJob::Output& o) {
    if (o.orient && !h2j_gpu_orient) return kNoStageMessage;
    return (finishing(o) && !(h2j_gpu_finish && h2j_gpu_jpeg2)) ? kNoFinishMessage : kNoRgbMessage;
}
// the outputs of a parsed job: every rendition's is resolved on its own, and invalid options fail that
// rendition alone
void resolve_outputs(const h2j_out_opts6* o, int nr, FrameJob& job) {
    job.nouts = nr;
    for (int r = 0; r < nr; r++) {
        job.outs[r] = FrameJob::Output();
        if (out_opts_valid(o[r])) job.outs[r] = resolve_output(o[r], job.hdr.out_w, job.hdr.out_h, job.sei_orient);
        else job.outs[r].error = H2J_ERR_OUT_OPTS;
        if (job.outs[r].error == 0 && job.outs[r].orient && !h2j_gpu_orient) job.outs[r].error = H2J_ERR_NO_STAGE;
        if (job.outs[r].error == 0 && finishing(job.outs[r]) && !(h2j_gpu_finish && h2j_gpu_jpeg2)) job.outs[r].error = H2J_ERR_NO_STAGE;
        if (job.outs[r].error == 0 && job.outs[r].format && !h2j_gpu_rgb) job.outs[r].error = H2J_ERR_NO_STAGE;
    }
}
// parse one item of a batch with the output options of its nr renditions (a plain item: one).  The item
// is not parsed when none is valid: it fails with the first one's message.  *ran: the entropy decode ran
int parse_item_multi(const uint8_t* d, size_t n, const h2j_out_opts6* o, int nr, FrameJob& job, bool* ran) {
    *ran = std::any_of(o, o + nr, out_opts_valid);
    if (!*ran) {
        job.clear();
        job.error = H2J_ERR_OUT_OPTS;
        job.message = out_opts_message(o[0]);
        return job.error;
    }
    const int rc = parse_any(d, n, job);
    if (rc == 0) resolve_outputs(o, nr, job);  // needs the parsed size
    return rc;
}

}  // namespace

// The events of a chunk, in the order its stream reaches them
enum {
    EV_BEGIN,       // before the H2D copy
    EV_H2D,         // after it; the wait for the other slot's kernels follows
    EV_GPU_BEGIN,   // after that wait: the chunk's GPU work starts with the arena fill
    EV_ZEROED,
    EV_K0,
    EV_K1,
    EV_K2,
    EV_K3,
    EV_SCALE,       // after K3o (oriented output), K3s / K3r / K3p (scaled output), K3u (finishing) and K3c (RGB output)
    EV_K4,
    EV_K5,          // the last kernel: the other slot's next chunk waits for it
    EV_STATS,       // after the stats D2H
    EV_PAY_BEGIN,   // around the in-stream payload D2H
    EV_PAY_END,
    EV_PAY2_BEGIN,  // around a second (whole) payload copy (sync)
    EV_PAY2_END,
    EV_END,
    EV_N
};

// One in-flight chunk: its stream, buffers and layout.
struct Slot {
    void* stream = nullptr;
    void* ev[EV_N] = {nullptr};
    size_t pay_pre = 0;        // payload bytes already copied in-stream by enqueue() (estimated, <= h_seg's capacity)
    size_t raw_off = 0;        // h_seg: the chunk's RGB region (plan.rgb_bytes) in front, the payloads from here (0: no raw output)
    bool raw_pre = false;      // the RGB region was copied in-stream by enqueue() (h_seg had room for it)
    int small_runs = 0;        // consecutive chunks whose payload used < 1/4 of h_seg (shrink after 8)
    size_t small_max = 0;      // the largest payload of that run
    DevBuf d_in, d_arena, d_seg, d_scratch;
    HostBuf h_in, h_js, h_seg;
    ChunkPlan plan;  // the chunk's frames and views, layouts and maps (chunk_plan.h)
    std::vector<int> live;  // job index of each frame of the chunk
    std::vector<FrameJob>* jobs = nullptr;  // the job set `live` indexes
    h2j_gpu_batch batch{};   // K0 .. K3, K3s / K3r / K3p: the frames
    h2j_gpu_batch jbatch{};  // K4, K5: the views (== batch when nv == nf)
    int stages = 0;
    bool entropy = false, pending = false;

    void release() {
        d_in.release();
        d_arena.release();
        d_seg.release();
        d_scratch.release();
        h_in.release();
        h_js.release();
        h_seg.release();
        for (auto& e : ev)
            if (e) h2j_gpu_event_destroy(e);
        if (stream) h2j_gpu_stream_destroy(stream);
        stream = nullptr;
    }
};

// stats slots (h2j_engine_stats): times in ms summed over chunks; ST_RECON is K1 only, ST_PREP is K0
// ST_PARSE: submission -> last picture parsed (includes waiting behind the previous batch's parse);
// ST_PARSE_RUN: first -> last picture parsed (the pool's time on this batch)
// ST_D2H_STATS / ST_D2H_PAY: the two parts of ST_D2H (per-picture jstat records; JPEG payloads),
// ST_PAY_BYTES: payload bytes produced, ST_PAY_COPIED: payload bytes moved (the in-stream copy moves
// the pinned buffer's capacity), ST_HOST_GROW: host ms spent growing the pinned payload buffer
// 
enum { ST_PARSE, ST_H2D, ST_RECON, ST_DEBLOCK, ST_SAO, ST_JPEG, ST_D2H, ST_ASSEMBLE, ST_TOTAL, ST_FRAMES, ST_BYTES,
       ST_ENTROPY, ST_PREP, ST_CHUNKS, ST_PACK, ST_PARSE_RUN, ST_D2H_STATS, ST_D2H_PAY, ST_PAY_BYTES, ST_HOST_GROW,
       ST_H2D_BYTES, ST_PAY_COPIED, ST_SCALE, ST_RENDITIONS, ST_PARSED, ST_RAW_BYTES, ST_N };  // ST_PACK: host time packing records into staging; ST_SCALE: K3o + K3s + K3r + K3p + K3u + K3c
// ST_RAW_BYTES: bytes of the raw (RGB) renditions delivered; K3c's time counts in ST_SCALE
// ST_RENDITIONS: JPEG outputs of the batch (ST_FRAMES: decoded pictures); ST_PARSED: pictures whose entropy decode ran

struct ChunkTime {
    int frames = 0;
    double k1_ms = 0, kernels_ms = 0;  // K1 launch; K0..K5 (HIP events on the chunk's stream)
};

// A submitted batch (h2j_engine_submit; h2j_engine_transcode is submit + wait).
struct Batch {
    int64_t ticket = 0;
    int n = 0;
    const uint8_t* const* data = nullptr;  // caller-owned until the batch is waited for
    const size_t* sizes = nullptr;
    uint8_t* out = nullptr;
    size_t out_cap = 0;
    size_t* out_off = nullptr;
    size_t* out_len = nullptr;
    int* status = nullptr;
    int32_t* out_wh = nullptr;                 // per rendition: its output's W, H (may be null)
    size_t raw_planned = 0;                    // bytes of the raw renditions the chunks planned so far hold
    std::vector<h2j_out_opts6> opts;           // output options per rendition, item-major (a plain item has one rendition)
    std::vector<int> rbase;                    // first rendition of each item, n + 1 entries
    int nout = 0;                              // entries of opts / out_off / out_len / status: rbase[n]
    std::atomic<int> nparsed{0};               // items whose entropy decode ran
    std::vector<int> bounds;                   // parse chunks: index ranges
    std::vector<int> chunk_of;
    std::unique_ptr<std::atomic<int>[]> left;  // pictures of each parse chunk still being parsed
    int jobset = -1;                           // Engine::jobsets slot the batch parses into
    bool parsed = false, done = false;
    int rc = 0;
    double t0 = 0, t_parse0 = 0, t_parsed = 0;
    // results handed to the caller by h2j_engine_wait (per ticket: a later batch that finishes
    // before this one is waited for does not overwrite them)
    double stats[ST_N] = {0};
    std::vector<ChunkTime> chunk_log;
    std::vector<std::string> msg;  // parse messages of the failed pictures
    std::string err;
};

struct Engine {
    int device = 0;
    ThreadPool* pool = nullptr;
    HostPlan plan;  // host threads / NUMA placement of the pool
    std::string err;
    std::vector<FrameJob> jobs;  // single-picture entry points (decode / jpeg_coeffs)
    // Asynchronous batches: a parser thread runs the pool over batch after batch, a driver thread
    // runs each batch's GPU chunks and JPEG assembly, so one batch's GPU tail overlaps the next
    // batch's entropy decoding.  At most two batches hold a job set at a time.
    std::mutex amu;
    std::condition_variable acv;
    std::deque<Batch*> parse_q, gpu_q;
    std::vector<std::unique_ptr<Batch>> batches;  // submitted and not yet waited for
    std::vector<FrameJob> jobsets[2];
    bool jobset_busy[2] = {false, false};
    int64_t next_ticket = 1;
    int active = 0;  // submitted batches not done
    bool stop = false;
    std::thread parser, driver;
    std::mutex pool_mu;  // held by whoever runs a parallel_for on the pool
    // results of the last batch a caller waited for (h2j_engine_wait copies them under amu; they
    // stay valid until the next wait returns)
    double last_stats[ST_N] = {0};
    std::vector<int> last_status;          // per-picture status
    std::vector<std::string> last_msg;     // ... and the parse messages of its failed pictures
    std::vector<ChunkTime> last_chunk_log;  // its chunks (h2j_engine_chunk_times)
    std::vector<ChunkTime> chunk_log;       // chunks of the batch being driven (driver thread)
    std::string derr;                       // error of the batch being driven (driver thread)
    Slot slot[2];
    double stats[ST_N] = {0};  // working stats of the batch being driven
    double slot_hbm_budget = 64e9;  // per slot; shared with the other engines on the device
    double pay_per_px = 0;          // JPEG payload bytes per output pixel, running estimate (both slots)
    bool strict_reference = false;  // H2J_STRICT_REFERENCE=1: fail where the reference returns false

    ~Engine() {
        {
            std::unique_lock<std::mutex> lk(amu);
            acv.wait(lk, [&] { return active == 0; });
            stop = true;
        }
        acv.notify_all();
        if (parser.joinable()) parser.join();
        if (driver.joinable()) driver.join();
        slot[0].release();
        slot[1].release();
        delete pool;
    }

    // run f(i), i < n, on the pool if no one else is using it (the parser), else on this thread
    void par(int n, const std::function<void(int)>& f) {
        if (pool_mu.try_lock()) {
            pool->parallel_for(n, f);
            pool_mu.unlock();
        } else {
            for (int i = 0; i < n; i++) f(i);
        }
    }
    void start_threads();
    void parse_loop();
    void drive_loop();
    int run_batch(Batch& b);
    // wait until no batch is in flight (the single-picture entry points use slot 0 directly)
    void quiesce() {
        std::unique_lock<std::mutex> lk(amu);
        acv.wait(lk, [&] { return active == 0; });
    }

    // the driver thread reports into the batch it drives (a caller may be reading `err`)
    int fail(const std::string& m) {
        if (driver.joinable() && std::this_thread::get_id() == driver.get_id()) derr = m;
        else err = m;
        return -1;
    }
    // an enqueue that fails after its first async operation: wait for what was queued on the
    // slot's stream, so the staging / device buffers are idle before anyone reuses or frees them
    int drain_fail(Slot& s, const std::string& m) {
        h2j_gpu_stream_sync(s.stream);
        return fail(m);
    }

    // Lay out, pack and enqueue the GPU work of jobs[live] on slot s.
    // stages: 1 recon, 2 +deblock, 3 +sao, 4 +jpeg forward path; entropy: +K5.
    // pool_free: the thread pool may be used for packing (not busy parsing).
    // `after`: the other slot, when its kernels are still in flight -- this slot's kernels start once
    // they have finished (its copies and the host's assembly still overlap them)
    int enqueue(Slot& s, int stages, bool entropy, bool pool_free = true, const Slot* after = nullptr);  // s.jobs must be set
    // enqueue's steps, after the plan (ChunkPlan): buffers, staging bytes, descriptors, launches, payload copy
    int ensure_buffers(Slot& s);
    void pack_staging(Slot& s, bool pool_free);
    void fill_descriptors(Slot& s);
    int launch(Slot& s, const Slot* after);
    int enqueue_payload_copy(Slot& s);
    // Wait for slot s and copy its payloads down (entropy chunks).
    int sync(Slot& s);
};

int Engine::ensure_buffers(Slot& s) {
    const ChunkPlan& p = s.plan;
    const std::string dev_failed = "device allocation failed: ";
    if (!s.h_in.ensure(p.at.bytes)) return fail("pinned host allocation failed");
    if (!s.d_in.ensure(p.at.bytes)) return fail(dev_failed + h2j_gpu_last_error());
    if (!s.d_arena.ensure(p.arena_bytes)) return fail(dev_failed + h2j_gpu_last_error());
    if (!s.entropy) return 0;
    if (!s.d_seg.ensure(p.seg_cap)) return fail(dev_failed + h2j_gpu_last_error());
    if (!s.d_scratch.ensure(static_cast<size_t>(p.nv) * p.tiles * 4 + 256)) return fail(dev_failed + h2j_gpu_last_error());
    if (!s.h_js.ensure(static_cast<size_t>(p.njstat) * p.jstat_stride + 256)) return fail("pinned host allocation failed");
    return 0;
}

// the chunk's upload: frames, maps, views and the jobs' records at their places (plan.at) in the pinned buffer
void Engine::pack_staging(Slot& s, bool pool_free) {
    const ChunkPlan& p = s.plan;
    uint8_t* hin = s.h_in.p;
    auto put = [&](size_t at, const void* src, size_t bytes) {
        if (bytes) std::memcpy(hin + at, src, bytes);
    };
    put(p.at.frames, p.frames.data(), p.nf * sizeof(h2j_frame));
    for (size_t j = 0; j < p.wins.size(); j++) {  // the windows' frame copies, behind the nf frames
        const h2j_frame wf = p.wframe(static_cast<int>(j));
        put(p.at.frames + (p.nf + j) * sizeof(h2j_frame), &wf, sizeof(wf));
    }
    put(p.at.k1map, p.k1map.data(), p.k1map.size() * 4);
    put(p.at.k1all, p.k1all.data(), p.k1all.size() * 4);
    put(p.at.sao, p.saomap.data(), p.saomap.size() * 4);
    put(p.at.k1map8, p.k1map8.data(), p.k1map8.size() * 4);
    put(p.at.k1hevc, p.k1hevc.data(), p.k1hevc.size() * 4);
    if (p.views) {
        h2j_frame* jv = reinterpret_cast<h2j_frame*>(hin + p.at.jframes);
        for (int v = 0; v < p.nv; v++) jv[v] = p.view(v);
        put(p.at.scale, p.scalemap.data(), p.scalemap.size() * sizeof(h2j_scaled));
        put(p.at.pyr, p.pyrmap.data(), p.pyrmap.size() * sizeof(h2j_pyramid));
        put(p.at.orient, p.orientmap.data(), p.orientmap.size() * sizeof(h2j_orient));
        put(p.at.finish, p.finmap.data(), p.finmap.size() * sizeof(h2j_finish));
    }
    if (p.qforced && !p.compact()) put(p.at.qforce, p.vqscale.data(), static_cast<size_t>(p.nv) * 4);
    if (p.compact()) {  // the views K4 / K5 run on, and their forced scales, packed
        h2j_frame* jc = reinterpret_cast<h2j_frame*>(hin + p.at.jcompact);
        int32_t* qf = reinterpret_cast<int32_t*>(hin + p.at.qforce);
        for (size_t i = 0; i < p.jviews.size(); i++) {
            jc[i] = p.view(p.jviews[i]);
            if (p.qforced) qf[i] = p.vqscale[p.jviews[i]];
        }
    }
    put(p.at.rgb, p.rgbmap.data(), p.rgbmap.size() * sizeof(h2j_rgb));
    const std::vector<FrameJob>& jobs = *s.jobs;
    auto pack = [&](int k) {  // the frame's record ranges are where plan_chunk numbered them
        const FrameJob& j = jobs[s.live[k]];
        const h2j_frame& f = p.frames[k];
        put(p.at.tus + f.tu * sizeof(h2j_tu), j.tus.data(), j.tus.size() * sizeof(h2j_tu));
        put(p.at.coefs + f.coef * sizeof(h2j_coef), j.coefs.data(), j.coefs.size() * sizeof(h2j_coef));
        put(p.at.ctbs + f.ctb * sizeof(h2j_ctb), j.ctbs.data(), j.ctbs.size() * sizeof(h2j_ctb));
        put(p.at.slices + f.slice * sizeof(h2j_slice), j.slices.data(), j.slices.size() * sizeof(h2j_slice));
        put(p.at.sl + f.sl, j.sl.data(), j.sl.size());
    };
    const double tp = now_ms();
    if (pool_free) par(p.nf, pack);
    else for (int k = 0; k < p.nf; k++) pack(k);
    stats[ST_PACK] += now_ms() - tp;
}

// the plan's descriptor with the device pointers of this slot's buffers
void Engine::fill_descriptors(Slot& s) {
    const ChunkPlan& p = s.plan;
    const uint8_t* din = static_cast<const uint8_t*>(s.d_in.p);
    uint8_t* scratch = static_cast<uint8_t*>(s.d_scratch.p);
    h2j_gpu_batch& b = s.batch;
    b = p.desc;
    b.frames = reinterpret_cast<const h2j_frame*>(din + p.at.frames);
    b.tus = reinterpret_cast<const h2j_tu*>(din + p.at.tus);
    b.coefs = reinterpret_cast<const h2j_coef*>(din + p.at.coefs);
    b.ctbs = reinterpret_cast<const h2j_ctb*>(din + p.at.ctbs);
    b.slices = reinterpret_cast<const h2j_slice*>(din + p.at.slices);
    b.sl = din + p.at.sl;
    b.k1map = reinterpret_cast<const uint32_t*>(din + p.at.k1map);
    b.k1all = reinterpret_cast<const uint32_t*>(din + p.at.k1all);
    b.k1map8 = reinterpret_cast<const uint32_t*>(din + p.at.k1map8);
    b.k1hevc = reinterpret_cast<const uint32_t*>(din + p.at.k1hevc);
    b.sao_map = reinterpret_cast<const uint32_t*>(din + p.at.sao);
    b.jframes = p.views ? reinterpret_cast<const h2j_frame*>(din + p.at.jframes) : b.frames;
    b.scale_map = !p.scalemap.empty() ? reinterpret_cast<const h2j_scaled*>(din + p.at.scale) : nullptr;
    b.pyr_map = !p.pyrmap.empty() ? reinterpret_cast<const h2j_pyramid*>(din + p.at.pyr) : nullptr;
    b.arena = static_cast<uint8_t*>(s.d_arena.p);
    b.jpeg_dense = s.entropy ? 0 : 1;
    b.seg = s.entropy ? static_cast<uint8_t*>(s.d_seg.p) : nullptr;
    b.seg_cap = s.entropy ? p.seg_cap : 0;
    b.seg_total = s.entropy ? reinterpret_cast<uint64_t*>(scratch) : nullptr;
    b.tile_bits = s.entropy ? reinterpret_cast<uint32_t*>(scratch + 256) : nullptr;
    // K4 / K5 read only the views and the arena: with several renditions of a frame they run on a
    // descriptor whose frames are the nv views (nv == nf: the one descriptor, as without renditions)
    h2j_gpu_batch& jb = s.jbatch;
    jb = b;
    if (p.nv > p.nf) {
        jb.nframes = p.nv;
        jb.frames = jb.jframes = b.jframes;
    }
    if (p.compact()) {  // ... and on those of them that get a JPEG, where some do not
        jb.nframes = p.njpeg;
        jb.frames = jb.jframes = reinterpret_cast<const h2j_frame*>(din + p.at.jcompact);
    }
}

// upload, the kernels of s.stages, and the stats download, on the slot's stream
int Engine::launch(Slot& s, const Slot* after) {
    const ChunkPlan& p = s.plan;
    const h2j_gpu_batch& b = s.batch;
    const h2j_gpu_batch& jb = s.jbatch;
    void* st = s.stream;
    int r = 0;
    r |= h2j_gpu_event_record(s.ev[EV_BEGIN], st);
    r |= h2j_gpu_memcpy_h2d(s.d_in.p, s.h_in.p, p.at.bytes, st);
    r |= h2j_gpu_event_record(s.ev[EV_H2D], st);
    stats[ST_H2D_BYTES] += static_cast<double>(p.at.bytes);
    // two GPU sub-chunks of one parsed range (4K batches, mixed batches past the slot's HBM budget)
    // would otherwise run their kernels side by side: the GPU is not the bound (the host entropy
    // threads are), and concurrent launches inflated every stage's event time and rocprof duration
    // (r05: 4K K4b 1.14 ms and the arena fill 1.18 ms per 256 pictures, 0.004 / 0.037 ms alone)
    if (after && after->pending) r |= h2j_gpu_stream_wait_event(st, after->ev[EV_K5]);
    r |= h2j_gpu_event_record(s.ev[EV_GPU_BEGIN], st);
    r |= h2j_gpu_memset(s.d_arena.p, 0, p.zero_bytes, st);
    r |= h2j_gpu_event_record(s.ev[EV_ZEROED], st);
    if (r) return drain_fail(s, std::string("upload failed: ") + h2j_gpu_last_error());
    if (h2j_gpu_prep(&b, st)) return drain_fail(s, h2j_gpu_last_error());
    h2j_gpu_event_record(s.ev[EV_K0], st);
    if (h2j_gpu_predict(&b, st)) return drain_fail(s, h2j_gpu_last_error());
    h2j_gpu_event_record(s.ev[EV_K1], st);
    if (s.stages >= 2 && h2j_gpu_deblock(&b, st)) return drain_fail(s, h2j_gpu_last_error());
    h2j_gpu_event_record(s.ev[EV_K2], st);
    if (s.stages >= 3 && h2j_gpu_sao(&b, st)) return drain_fail(s, h2j_gpu_last_error());
    h2j_gpu_event_record(s.ev[EV_K3], st);
    // K3o: only in chunks with oriented sources (they exist only when the kernel library has the stage)
    if (s.stages >= 3 && !p.orientmap.empty() &&
        (!h2j_gpu_orient || h2j_gpu_orient(&b, reinterpret_cast<const h2j_orient*>(static_cast<const uint8_t*>(s.d_in.p) + p.at.orient),
                                           p.orient_first, p.orient_count, p.orient_tiles, st)))
        return drain_fail(s, h2j_gpu_orient ? h2j_gpu_last_error() : kNoStageMessage);
    if (s.stages >= 3 && h2j_gpu_scale(&b, st)) return drain_fail(s, h2j_gpu_last_error());  // K3s, K3r: no launch without scaled pictures
    // K3u: only in chunks with sharpened outputs (they exist only when the kernel library has the stage)
    if (s.stages >= 3 && !p.finmap.empty() &&
        (!h2j_gpu_finish || h2j_gpu_finish(&b, reinterpret_cast<const h2j_finish*>(static_cast<const uint8_t*>(s.d_in.p) + p.at.finish),
                                           p.fin_first, p.fin_count, p.fin_tiles, st)))
        return drain_fail(s, h2j_gpu_finish ? h2j_gpu_last_error() : kNoFinishMessage);
    // K3c: only in chunks with raw outputs (likewise); out of place, K4 reads what it read
    if (s.stages >= 3 && !p.rgbmap.empty() &&
        (!h2j_gpu_rgb || h2j_gpu_rgb(&b, reinterpret_cast<const h2j_rgb*>(static_cast<const uint8_t*>(s.d_in.p) + p.at.rgb),
                                     p.rgb_first, p.rgb_count, p.rgb_tiles, st)))
        return drain_fail(s, h2j_gpu_rgb ? h2j_gpu_last_error() : kNoRgbMessage);
    h2j_gpu_event_record(s.ev[EV_SCALE], st);
    // a chunk of raw renditions only: nobody asked for a JPEG, so no K4 / K5 and no payload (the pool's byte count,
    // which K5 would have written, is cleared instead)
    const bool jpegs = p.njpeg > 0;
    // K4: through h2j_gpu_jpeg2 only in chunks with a forced quantiser scale (likewise)
    if (s.stages >= 4 && jpegs && p.qforced) {
        if (!h2j_gpu_jpeg2 || h2j_gpu_jpeg2(&jb, reinterpret_cast<const int32_t*>(static_cast<const uint8_t*>(s.d_in.p) + p.at.qforce), st))
            return drain_fail(s, h2j_gpu_jpeg2 ? h2j_gpu_last_error() : kNoFinishMessage);
    } else if (s.stages >= 4 && jpegs && h2j_gpu_jpeg(&jb, st)) return drain_fail(s, h2j_gpu_last_error());
    h2j_gpu_event_record(s.ev[EV_K4], st);
    if (s.entropy && jpegs && h2j_gpu_entropy(&jb, st)) return drain_fail(s, h2j_gpu_last_error());
    if (s.entropy && !jpegs && h2j_gpu_memset(s.d_scratch.p, 0, 8, st)) return drain_fail(s, h2j_gpu_last_error());
    h2j_gpu_event_record(s.ev[EV_K5], st);
    if (s.entropy) {
        r |= h2j_gpu_memcpy_d2h(s.h_js.p, s.d_scratch.p, 8, st);  // seg_total
        r |= h2j_gpu_memcpy_d2h(s.h_js.p + 256, static_cast<uint8_t*>(s.d_arena.p) + p.jstat_base,
                                static_cast<size_t>(p.njstat) * p.jstat_stride, st);
        if (r) return drain_fail(s, std::string("download failed: ") + h2j_gpu_last_error());
    }
    h2j_gpu_event_record(s.ev[EV_STATS], st);
    return 0;
}

// the payloads follow in the same stream, sized by the pinned buffer (1.25x the largest total
// seen): no host round trip between the kernels and the copy.  r04/r05 enqueued the copy in
// sync() once the host had read the total: at 4K its interval measured 40-78 ms per step for
// 121 MB against 4 ms for the bare copy (tools/d2h_probe: 30 GB/s pinned) -- the submitting
// driver thread waited for CPU behind the 16 entropy threads (profiles/r05_4k_d2h.md).  A
// total above the capacity (first chunks, growth) is copied again whole in sync().
int Engine::enqueue_payload_copy(Slot& s) {
    if (s.small_runs >= 8) {  // the slot's last chunk has been assembled: h_seg is free to go
        const double tg = now_ms();
        const size_t keep = s.small_max + s.small_max / 4 + 16;
        s.h_seg.release();
        if (!s.h_seg.ensure(keep)) return fail("pinned host allocation failed");
        stats[ST_HOST_GROW] += now_ms() - tg;
        s.small_runs = 0;
    }
    s.pay_pre = 0;
    // raw outputs: the chunk's RGB region goes in front of the payloads, by the same copy policy -- in-stream when
    // the pinned buffer already holds it (the plan knows its size), else in sync(), where the buffer grows
    const size_t raw = s.entropy ? s.plan.rgb_bytes : 0;
    s.raw_off = raw;
    s.raw_pre = false;
    if (s.entropy && s.h_seg.cap > raw) {
        // the copy is sized by the engine's payload-per-pixel estimate (1.3x, 4 KB
        // granules), not by the buffer's high-water mark: a small chunk after a 4K one moves its own
        // few MB, not the 4K chunk's 150 MB
        size_t want = s.plan.seg_cap;
        if (pay_per_px > 0) want = (static_cast<size_t>(1.3 * pay_per_px * s.plan.px) + 65536 + 4095) & ~static_cast<size_t>(4095);
        s.pay_pre = s.plan.njpeg > 0 ? std::min(std::min(s.h_seg.cap - raw, s.plan.seg_cap), want) : 0;  // raw renditions only: no payload
        h2j_gpu_event_record(s.ev[EV_PAY_BEGIN], s.stream);
        if (raw) {
            if (h2j_gpu_memcpy_d2h(s.h_seg.p, static_cast<uint8_t*>(s.d_arena.p) + s.plan.rgb_base, raw, s.stream))
                return drain_fail(s, std::string("download failed: ") + h2j_gpu_last_error());
            s.raw_pre = true;
        }
        if (s.pay_pre && h2j_gpu_memcpy_d2h(s.h_seg.p + raw, s.d_seg.p, s.pay_pre, s.stream))
            return drain_fail(s, std::string("download failed: ") + h2j_gpu_last_error());
        h2j_gpu_event_record(s.ev[EV_PAY_END], s.stream);
    }
    return 0;
}

int Engine::enqueue(Slot& s, int stages, bool entropy, bool pool_free, const Slot* after) {
    s.stages = stages;
    s.entropy = entropy;
    s.pending = false;
    if (s.live.empty()) return 0;
    plan_chunk(*s.jobs, s.live, s.plan);
    if (ensure_buffers(s)) return -1;
    pack_staging(s, pool_free);
    fill_descriptors(s);
    if (launch(s, after) || enqueue_payload_copy(s)) return -1;
    s.pending = true;
    double bytes = 0;
    for (const h2j_frame& f : s.plan.frames) bytes += 1.5 * f.out_w * f.out_h * (4.0 + (f.bit_depth > 8 ? 2.0 : 1.0));
    stats[ST_BYTES] += bytes;
    return 0;
}

int Engine::sync(Slot& s) {
    if (!s.pending) return 0;
    s.pending = false;
    if (h2j_gpu_stream_sync(s.stream)) return fail(std::string("GPU execution failed: ") + h2j_gpu_last_error());
    bool pay_late = false;
    if (s.entropy) {
        uint64_t total = 0;
        std::memcpy(&total, s.h_js.p, 8);
        stats[ST_PAY_BYTES] += static_cast<double>(total);
        if (s.plan.px > 0 && s.plan.njpeg > 0) {  // payload per pixel: a running mean, never below the last chunk's
            const double ratio = static_cast<double>(total) / s.plan.px;
            pay_per_px = pay_per_px > 0 ? std::max(ratio, 0.7 * pay_per_px + 0.3 * ratio) : ratio;
        }
        stats[ST_PAY_COPIED] += static_cast<double>(s.pay_pre + (s.raw_pre ? s.raw_off : 0));  // the in-stream copy, used or not (the RGB region with it)
        const size_t raw = s.raw_off;
        if (total > s.pay_pre || (raw && !s.raw_pre)) {  // not (all) copied in-stream: grow with headroom, copy it whole
            const double tg = now_ms();
            if (!s.h_seg.ensure(raw + total + total / 4 + 16)) return fail("pinned host allocation failed");
            stats[ST_HOST_GROW] += now_ms() - tg;
            stats[ST_PAY_COPIED] += static_cast<double>(raw + total);
            pay_late = true;
            h2j_gpu_event_record(s.ev[EV_PAY2_BEGIN], s.stream);
            // (the RGB region again too: the buffer may be a new one)
            if ((raw && h2j_gpu_memcpy_d2h(s.h_seg.p, static_cast<uint8_t*>(s.d_arena.p) + s.plan.rgb_base, raw, s.stream)) ||
                (total && h2j_gpu_memcpy_d2h(s.h_seg.p + raw, s.d_seg.p, total, s.stream)))
                return fail(std::string("download failed: ") + h2j_gpu_last_error());
            h2j_gpu_event_record(s.ev[EV_PAY2_END], s.stream);
        }
        // the pinned buffer shrinks after 8 chunks in a row that used less than a quarter of it
        if ((raw + total) * 4 < s.h_seg.cap) {
            s.small_max = s.small_runs ? std::max(s.small_max, static_cast<size_t>(raw + total)) : static_cast<size_t>(raw + total);
            s.small_runs++;
        } else {
            s.small_runs = 0;
        }
    }
    if (h2j_gpu_event_record(s.ev[EV_END], s.stream) || h2j_gpu_stream_sync(s.stream))
        return fail(std::string("download failed: ") + h2j_gpu_last_error());
    // the H2D copy alone; the arena fill (after any wait for the other slot's kernels) counts with K0
    stats[ST_H2D] += h2j_gpu_event_elapsed_ms(s.ev[EV_BEGIN], s.ev[EV_H2D]);
    stats[ST_PREP] += h2j_gpu_event_elapsed_ms(s.ev[EV_GPU_BEGIN], s.ev[EV_K0]);
    stats[ST_RECON] += h2j_gpu_event_elapsed_ms(s.ev[EV_K0], s.ev[EV_K1]);
    stats[ST_CHUNKS] += 1;
    stats[ST_DEBLOCK] += h2j_gpu_event_elapsed_ms(s.ev[EV_K1], s.ev[EV_K2]);
    stats[ST_SAO] += h2j_gpu_event_elapsed_ms(s.ev[EV_K2], s.ev[EV_K3]);
    stats[ST_SCALE] += h2j_gpu_event_elapsed_ms(s.ev[EV_K3], s.ev[EV_SCALE]);
    stats[ST_JPEG] += h2j_gpu_event_elapsed_ms(s.ev[EV_SCALE], s.ev[EV_K4]);
    stats[ST_ENTROPY] += h2j_gpu_event_elapsed_ms(s.ev[EV_K4], s.ev[EV_K5]);
    // copies only (the payload copy is enqueued once the host has read the sizes)
    const double d2h_stats = h2j_gpu_event_elapsed_ms(s.ev[EV_K5], s.ev[EV_STATS]);
    // both payload copies when the in-stream one fell short (the second one's events had
    // overwritten the first's)
    const double d2h_pay = (s.entropy && (s.pay_pre || s.raw_pre) ? h2j_gpu_event_elapsed_ms(s.ev[EV_PAY_BEGIN], s.ev[EV_PAY_END]) : 0.0) +
                           (pay_late ? h2j_gpu_event_elapsed_ms(s.ev[EV_PAY2_BEGIN], s.ev[EV_PAY2_END]) : 0.0);
    stats[ST_D2H] += d2h_stats + d2h_pay;
    stats[ST_D2H_STATS] += d2h_stats;
    stats[ST_D2H_PAY] += d2h_pay;
    ChunkTime ct;
    ct.frames = static_cast<int>(s.live.size());
    ct.k1_ms = h2j_gpu_event_elapsed_ms(s.ev[EV_K0], s.ev[EV_K1]);
    ct.kernels_ms = h2j_gpu_event_elapsed_ms(s.ev[EV_GPU_BEGIN], s.ev[EV_K5]);
    chunk_log.push_back(ct);
    return 0;
}

// Chunk boundaries: chunks large enough to fill the GPU (K1 runs one
// workgroup per picture), small enough that parse / GPU / assembly overlap;
// the last quarter is split into shrinking chunks so that the GPU work left
// after the last picture is parsed (the pipeline's tail) is short.
std::vector<int> chunk_bounds(int n) {
    int chunk = n >= 512 ? 256 : n;
    const char* e = std::getenv("H2J_CHUNK");
    if (e && std::atoi(e) > 0) chunk = std::atoi(e);
    chunk = std::max(1, chunk);
    const char* tail = std::getenv("H2J_TAIL");  // "0": no shrinking tail chunks
    const bool shrink = !(tail && tail[0] == '0');
    const char* tmin = std::getenv("H2J_TAIL_MIN");  // smallest tail chunk (default 128: 256,256,256,128,128 for 1024)
    const int tail_min = tmin && std::atoi(tmin) > 0 ? std::atoi(tmin) : 128;
    std::vector<int> starts;
    int i = 0;
    while (i < n) {
        starts.push_back(i);
        int c = chunk;
        const int left = n - i;
        if (shrink && left <= chunk && left > tail_min && chunk >= 128) c = left / 2;  // tail: halve
        i += std::min(c, left);
    }
    starts.push_back(n);
    return starts;
}

// Throughput plan (asynchronous batches): one parse chunk of up to 1024 pictures (K1 runs up to
// four pictures per workgroup on launches that large); the GPU tail of a batch is hidden behind
// the next batch's entropy decoding instead of being cut into shrinking chunks.
std::vector<int> chunk_bounds_throughput(int n) {
    int chunk = 1024;
    const char* e = std::getenv("H2J_CHUNK_ASYNC");
    if (e && std::atoi(e) > 0) chunk = std::atoi(e);
    std::vector<int> starts;
    for (int i = 0; i < n; i += chunk) starts.push_back(i);
    starts.push_back(n);
    return starts;
}

// GPU sub-chunks of a parsed range are bounded by an HBM estimate per slot (pictures, residual,
// JPEG symbol tiles, payload pool: ~20 B per luma sample at 8 bits) and by 1024 pictures.
constexpr double kSlotHbmBudget = 64e9;  // at most, per slot (two slots per engine)
constexpr int kMaxGpuChunk = 1024;
static double hbm_estimate(const FrameJob& j) {
    const double px = static_cast<double>(j.hdr.width) * j.hdr.height;
    // (a scaled picture's 8-bit planes add 1.5 / 4^k B per sample, a resized picture's 1.5 W_o H_o B; its
    // JPEG regions shrink by more)
    const FrameJob::Output o0 = j.nouts ? j.outs[0] : FrameJob::Output();  // the first output (none: a failed job)
    const double opx0 = o0.windowed ? static_cast<double>(o0.win_w) * o0.win_h : px;  // the output's source: a window, or the picture
    const double spic = o0.scale_log2 == H2J_SCALE_RESAMPLE ? 1.5 * o0.fit_w * o0.fit_h : o0.scale_log2 ? 1.5 * opx0 / (1 << 2 * o0.scale_log2) : 0.0;
    double est = px * (j.hdr.bit_depth > 8 ? 24.0 : 20.0) + spic + (1 << 20);
    // several renditions: each output beyond the first adds its 8-bit planes (1.5 B per output sample), its
    // jcoef / tile region and its share of the payload pool (272 B per 8x8 block each: 6.4 B per sample),
    // and its jstat and tile_bits (a few KB)
    for (int r = 1; r < j.nouts; r++) {
        const FrameJob::Output& o = j.outs[r];
        if (o.error) continue;
        const double opx = o.scale_log2 == H2J_SCALE_RESAMPLE ? static_cast<double>(o.fit_w) * o.fit_h
                                                               : static_cast<double>(o.win_w) * o.win_h / (1 << 2 * o.scale_log2);
        est += 14.5 * opx + 8192;
    }
    // oriented sources: the planes K3o writes, in the picture's sample type, once per distinct orientation
    int oriented = 0;
    for (int r = 0; r < j.nouts; r++)
        if (j.outs[r].error == 0 && j.outs[r].orient && !((oriented >> j.outs[r].orient) & 1)) {
            oriented |= 1 << j.outs[r].orient;
            est += 1.5 * j.hdr.out_w * j.hdr.out_h * (j.hdr.bit_depth > 8 ? 2.0 : 1.0) + 4096;
        }
    // sharpened outputs: the 8-bit planes K3u writes (1.5 B per output sample)
    for (int r = 0; r < j.nouts; r++) {
        const FrameJob::Output& o = j.outs[r];
        if (o.error || !o.sharpen) continue;
        est += 1.5 * (o.scale_log2 == H2J_SCALE_RESAMPLE ? static_cast<double>(o.fit_w) * o.fit_h
                                                           : static_cast<double>(o.win_w) * o.win_h / (1 << 2 * o.scale_log2)) + 4096;
    }
    // raw outputs: the pixels K3c writes (3 B per output sample; one that shares a JPEG rendition's view added that
    // view's regions above for nothing: an overestimate)
    for (int r = 0; r < j.nouts; r++)
        if (j.outs[r].error == 0 && j.outs[r].format) est += 3.0 * j.outs[r].out_w() * j.outs[r].out_h() + 4096;
    return est;
}
// JPEG outputs of a job (at least one: the chunk bound counts a failed item as one)
static int views_estimate(const FrameJob& j) { return std::max(1, j.nouts); }

void Engine::start_threads() {
    std::lock_guard<std::mutex> g(amu);
    if (parser.joinable()) return;
    parser = std::thread([this] { parse_loop(); });
    driver = std::thread([this] { drive_loop(); });
}

void Engine::parse_loop() {
    for (;;) {
        Batch* b = nullptr;
        {
            std::unique_lock<std::mutex> lk(amu);
            acv.wait(lk, [&] { return stop || !parse_q.empty(); });
            if (parse_q.empty()) return;
            b = parse_q.front();
            parse_q.pop_front();
            acv.wait(lk, [&] { return !jobset_busy[0] || !jobset_busy[1]; });
            b->jobset = jobset_busy[0] ? 1 : 0;
            jobset_busy[b->jobset] = true;
        }
        b->t_parse0 = now_ms();
        std::vector<FrameJob>& jobs = jobsets[b->jobset];
        if (static_cast<int>(jobs.size()) < b->n) jobs.resize(static_cast<size_t>(b->n));
        // batches smaller than the thread pool (a lone IDecoder call): pictures with several
        // independent slices / WPP rows / tiles parse them on several threads
        const int slice_threads = std::max(1, (pool->size() + 1) / std::max(1, b->n));
        // inside each chunk the largest bitstreams start first (the threads then finish a chunk
        // together instead of idling behind one large picture); chunks keep their order
        std::vector<int> order(static_cast<size_t>(b->n));
        for (int i = 0; i < b->n; i++) order[i] = i;
        for (size_t c = 0; c + 1 < b->bounds.size(); c++)
            std::stable_sort(order.begin() + b->bounds[c], order.begin() + b->bounds[c + 1],
                             [&](int x, int y) { return b->sizes[x] > b->sizes[y]; });
        {
            std::lock_guard<std::mutex> g(pool_mu);
            pool->parallel_for(b->n, [&](int k) {
                const int i = order[static_cast<size_t>(k)];
                jobs[i].threads = slice_threads;
                bool ran = false;
                parse_item_multi(b->data[i], b->sizes[i], b->opts.data() + b->rbase[i], b->rbase[i + 1] - b->rbase[i], jobs[i], &ran);
                if (ran) b->nparsed.fetch_add(1, std::memory_order_relaxed);
                jobs[i].out_base = b->rbase[i];
                if (b->left[b->chunk_of[i]].fetch_sub(1) == 1) {
                    std::lock_guard<std::mutex> g2(amu);
                    acv.notify_all();
                }
            });
        }
        std::lock_guard<std::mutex> g(amu);
        b->t_parsed = now_ms();
        b->parsed = true;
        acv.notify_all();
    }
}

void Engine::drive_loop() {
    h2j_gpu_set_device(device);  // HIP's current device is per thread
    for (;;) {
        Batch* b = nullptr;
        {
            std::unique_lock<std::mutex> lk(amu);
            acv.wait(lk, [&] { return stop || !gpu_q.empty(); });
            if (gpu_q.empty()) return;
            b = gpu_q.front();
            gpu_q.pop_front();
        }
        derr.clear();
        const int rc = run_batch(*b);
        std::unique_lock<std::mutex> lk(amu);
        acv.wait(lk, [&] { return b->parsed; });  // a failed batch may still be parsing
        std::vector<FrameJob>* jobs = b->jobset >= 0 ? &jobsets[b->jobset] : nullptr;
        stats[ST_PARSE] = b->t_parsed > 0 ? b->t_parsed - b->t0 : 0;
        stats[ST_PARSE_RUN] = b->t_parsed > 0 ? b->t_parsed - b->t_parse0 : 0;
        stats[ST_TOTAL] = now_ms() - b->t0;
        stats[ST_PARSED] = b->nparsed.load();
        std::memcpy(b->stats, stats, sizeof(stats));
        b->chunk_log = chunk_log;
        b->err = derr;
        b->msg.assign(static_cast<size_t>(b->nout), std::string());
        if (jobs)
            for (int i = 0; i < b->n; i++) {
                for (int o = b->rbase[i]; o < b->rbase[i + 1]; o++) {
                    if (b->status[o] == 0) continue;
                    if ((*jobs)[i].error != 0) b->msg[o] = (*jobs)[i].message;
                    else if (b->status[o] == H2J_ERR_OUT_OPTS) b->msg[o] = out_opts_message(b->opts[static_cast<size_t>(o)], (*jobs)[i].hdr.out_w, (*jobs)[i].hdr.out_h, (*jobs)[i].sei_orient);
                    else if (b->status[o] == H2J_ERR_NO_STAGE) b->msg[o] = no_stage_message((*jobs)[i].outs[o - b->rbase[i]]);
                }
            }
        if (b->jobset >= 0) jobset_busy[b->jobset] = false;
        b->rc = rc;
        b->done = true;
        active--;
        acv.notify_all();
    }
}

// The GPU side of one batch (driver thread): as parse chunks complete, their pictures go to the
// two slots in GPU sub-chunks (HBM budget); slot c+1 is enqueued before slot c is assembled, so
// the GPU runs one sub-chunk while the host writes the JPEGs of the previous one.
int Engine::run_batch(Batch& b) {
    for (auto& v : stats) v = 0;
    chunk_log.clear();
    const int nchunks = static_cast<int>(b.bounds.size()) - 1;
    if (b.n == 0 || nchunks <= 0) return 0;
    size_t pos = 0;
    int rc = 0;
    int* status = b.status;
    auto assemble = [&](Slot& s) -> int {
        if (sync(s)) return -2;
        const double ta = now_ms();
        const ChunkPlan& p = s.plan;
        const int nf = p.nf, nv = p.nv, nr = static_cast<int>(p.rends.size());
        const uint8_t* js = s.h_js.p + 256;
        std::vector<size_t> sz(nv);  // per view: its JPEG, encoded once
        const uint8_t* pay = s.h_seg.p + s.raw_off;  // the payloads, behind the chunk's RGB region (raw outputs)
        auto size_of = [&](int k) {
            const h2j_jstat* st = reinterpret_cast<const h2j_jstat*>(js + k * p.jstat_stride);
            // (a view that only raw renditions show: K4 / K5 made a JPEG of it that nobody asked for; it is not assembled)
            sz[k] = (st->seg_off == ~0ull || !p.vjpeg[k]) ? 0 : jpeg_container_size(*st, pay + st->seg_off, kLavcIdent);
        };
        par(nv, size_of);
        // every rendition gets its place in the output; renditions of one view (the same resolved output)
        // hold the same bytes: the first is written, the others copied from it
        std::vector<size_t> at(nr);
        std::vector<int> first(nv, -1);  // per view: its first rendition with a place
        for (int q = 0; q < nr; q++) {
            const int i = p.rends[q].out, k = p.rends[q].view;
            // a device-side failure (e.g. a K1 band hand-off timed out) is recorded in the frame's own jstat
            const h2j_jstat* stf = reinterpret_cast<const h2j_jstat*>(js + p.fstat[p.scaled[k].frame] * p.jstat_stride);
            at[q] = ~static_cast<size_t>(0);
            if (stf->dev_error) {
                status[i] = -52;
                rc = -3;
                continue;
            }
            const int g = p.rends[q].rgb;  // a raw rendition: 3 W H pixel bytes from the chunk's RGB region
            const size_t len = g >= 0 ? 3 * static_cast<size_t>(p.rgbs[g].w) * p.rgbs[g].h : sz[k];
            if (!len) {
                status[i] = -51;  // payload pool overflow
                rc = -3;
                continue;
            }
            if (pos + len > b.out_cap) {
                status[i] = -50;
                rc = -3;
                continue;
            }
            at[q] = pos;
            if (g < 0 && first[k] < 0) first[k] = q;
            b.out_off[i] = pos;
            b.out_len[i] = len;
            pos += len;
        }
        auto write = [&](int k) {
            if (first[k] < 0) return;
            const h2j_jstat* st = reinterpret_cast<const h2j_jstat*>(js + k * p.jstat_stride);
            const h2j_scaled& sc = p.scaled[k];
            jpeg_write_container(*st, pay + st->seg_off, sc.jpeg_w, sc.jpeg_h, kLavcIdent, b.out + at[first[k]]);
        };
        par(nv, write);
        if (nr > nv || !p.rgbs.empty())
            for (int q = 0; q < nr; q++) {
                const int k = p.rends[q].view;
                if (p.rends[q].rgb < 0 && at[q] != ~static_cast<size_t>(0) && first[k] != q) std::memcpy(b.out + at[q], b.out + at[first[k]], sz[k]);
            }
        if (!p.rgbs.empty()) {  // the raw renditions' pixels: from the pinned buffer to their places
            par(nr, [&](int q) {
                const int g = p.rends[q].rgb;
                if (g < 0 || at[q] == ~static_cast<size_t>(0)) return;
                std::memcpy(b.out + at[q], s.h_seg.p + (p.rgbs[g].dst_off - p.rgb_base), b.out_len[p.rends[q].out]);
            });
            for (int q = 0; q < nr; q++)
                if (p.rends[q].rgb >= 0 && at[q] != ~static_cast<size_t>(0)) stats[ST_RAW_BYTES] += static_cast<double>(b.out_len[p.rends[q].out]);
        }
        stats[ST_ASSEMBLE] += now_ms() - ta;
        stats[ST_RENDITIONS] += nr;
        stats[ST_FRAMES] += nf;
        return 0;
    };
    int fail = 0, sc = 0;
    for (int c = 0; c < nchunks && !fail; c++) {
        {
            std::unique_lock<std::mutex> lk(amu);
            acv.wait(lk, [&] { return b.left[c].load() == 0; });
        }
        std::vector<FrameJob>& jobs = jobsets[b.jobset];
        int i = b.bounds[c];
        const int end = b.bounds[c + 1];
        // equal shares of the range's HBM estimate, as few as the budget allows (uneven splits
        // leave small, latency-bound launches behind)
        double total = 0;
        for (int k = i; k < end; k++) total += hbm_estimate(jobs[k]);
        const double budget = slot_hbm_budget;
        int range_views = 0;
        for (int k = i; k < end; k++) range_views += views_estimate(jobs[k]);
        const int parts = std::max(static_cast<int>(std::ceil(total / budget)),
                                   (range_views + kMaxGpuChunk - 1) / kMaxGpuChunk);
        const double share = total / std::max(1, parts);
        while (i < end && !fail) {
            int j = i;
            double est = 0;
            int nviews = 0;  // renditions count towards the chunk's size; an item's renditions stay together
            while (j < end && j - i < kMaxGpuChunk) {
                const double cst = hbm_estimate(jobs[j]);
                if (j > i && (est + cst > budget || est + cst / 2 > share || nviews + views_estimate(jobs[j]) > kMaxGpuChunk)) break;
                est += cst;
                nviews += views_estimate(jobs[j]);
                j++;
            }
            Slot& s = slot[sc & 1];
            if (s.pending && assemble(s)) { fail = 1; break; }
            s.live.clear();
            s.jobs = &jobs;
            for (int k = i; k < j; k++) {
                if (strict_reference && jobs[k].error == 0 && jobs[k].reorder_delay) {
                    // the reference sends one packet and never flushes: avcodec_receive_frame gives
                    // EAGAIN for a stream with output reordering and H265ToJpeg returns false
                    // (/root/reference/src/Decoder.cpp:324, 342-360)
                    jobs[k].error = -7;
                    jobs[k].message = "decoder delay: no picture before a flush (H2J_STRICT_REFERENCE)";
                }
                if (strict_reference && jobs[k].error == 0 && jobs[k].field_pair) {
                    // one packet holds one field: FFmpeg waits for the second field and the
                    // reference returns false (/root/reference/src/Decoder.cpp:324, 342-360)
                    jobs[k].error = -3;
                    jobs[k].message = "field picture (PAFF): no frame from one field (H2J_STRICT_REFERENCE)";
                }
                // a failed item fails every rendition; else each rendition's own options decide
                for (int o = b.rbase[k]; o < b.rbase[k + 1]; o++) {
                    if (jobs[k].error) {
                        status[o] = jobs[k].error;
                        continue;
                    }
                    FrameJob::Output& jo = jobs[k].outs[o - b.rbase[k]];
                    if (b.out_wh && jo.error != H2J_ERR_OUT_OPTS) {  // the options resolved: the output's size
                        b.out_wh[2 * o] = jo.out_w();
                        b.out_wh[2 * o + 1] = jo.out_h();
                    }
                    // a raw rendition's size is known here: one that cannot fit the output buffer behind the raw
                    // renditions planned before it (JPEGs only take more) fails now, and K3c does not run for it
                    if (jo.error == 0 && jo.format) {
                        const size_t len = 3 * static_cast<size_t>(jo.out_w()) * jo.out_h();
                        if (b.raw_planned + len > b.out_cap) {
                            jo.error = -50;
                            rc = -3;
                        } else {
                            b.raw_planned += len;
                        }
                    }
                    status[o] = jo.error;
                }
                // a parsed item none of whose renditions is valid (every window outside the picture) has no
                // view: it gets no frame in the chunk, its renditions have their statuses
                bool any_output = false;
                for (int r = 0; r < jobs[k].nouts; r++) any_output = any_output || jobs[k].outs[r].error == 0;
                if (jobs[k].error == 0 && any_output) s.live.push_back(k);
            }
            Slot& prev = slot[(sc + 1) & 1];
            if (enqueue(s, 4, true, true, &prev)) { fail = 1; break; }
            if (sc > 0 && prev.pending && assemble(prev)) { fail = 1; break; }
            sc++;
            i = j;
        }
    }
    for (int k = 0; k < 2 && !fail; k++) {
        Slot& s = slot[(sc + k) & 1];
        if (s.pending && assemble(s)) fail = 1;
    }
    if (fail) {
        for (auto& s : slot)
            if (s.pending) sync(s);
        return -2;
    }
    if (rc) derr = "output buffer too small or payload pool overflow";
    return rc;
}

}  // namespace h2j

using h2j::Engine;
using h2j::Slot;

struct h2j_engine {
    Engine e;
};

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

// submit one batch; latency: the synchronous plan (small tail chunks), else the throughput plan.
// Item i has nrend[i] renditions (null: one each); opts and the output arrays are item-major over all of
// them (opts null: the decoded size)
static int64_t submit_batch(h2j_engine* w, int n, const uint8_t* const* data, const size_t* sizes, const int32_t* nrend,
                            const h2j_out_opts6* opts, uint8_t* out, size_t out_cap, size_t* out_off, size_t* out_len,
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
    else b->opts.assign(static_cast<size_t>(b->nout), h2j::kPlainOutput);
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

int64_t h2j_engine_submit(h2j_engine* w, int n, const uint8_t* const* data, const size_t* sizes, uint8_t* out,
                          size_t out_cap, size_t* out_off, size_t* out_len, int* status) {
    if (!w || n < 0) return -1;
    return submit_batch(w, n, data, sizes, nullptr, nullptr, out, out_cap, out_off, out_len, status, false);
}

int64_t h2j_engine_submit_opts(h2j_engine* w, int n, const uint8_t* const* data, const size_t* sizes,
                               const h2j_out_opts* opts, uint8_t* out, size_t out_cap, size_t* out_off, size_t* out_len,
                               int* status) {
    if (!w || n < 0) return -1;
    return submit_batch(w, n, data, sizes, nullptr, h2j::opts6_of(n, opts).data(), out, out_cap, out_off, out_len, status, false);
}

int64_t h2j_engine_submit_opts2(h2j_engine* w, int n, const uint8_t* const* data, const size_t* sizes,
                                const h2j_out_opts2* opts, uint8_t* out, size_t out_cap, size_t* out_off,
                                size_t* out_len, int* status) {
    if (!w || n < 0) return -1;
    return submit_batch(w, n, data, sizes, nullptr, opts ? h2j::opts6_of(n, opts).data() : nullptr, out, out_cap, out_off, out_len, status, false);
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
    const int64_t t = submit_batch(w, n, data, sizes, nullptr, h2j::opts6_of(n, opts).data(), out, out_cap, out_off, out_len, status, true);
    return h2j_engine_wait(w, t);
}

int h2j_engine_transcode_opts2(h2j_engine* w, int n, const uint8_t* const* data, const size_t* sizes,
                               const h2j_out_opts2* opts, uint8_t* out, size_t out_cap, size_t* out_off,
                               size_t* out_len, int* status) {
    if (!w || n < 0) return -1;
    const int64_t t = submit_batch(w, n, data, sizes, nullptr, opts ? h2j::opts6_of(n, opts).data() : nullptr, out, out_cap, out_off, out_len, status, true);
    return h2j_engine_wait(w, t);
}

// nrend[i] in 1..H2J_MAX_RENDITIONS for every item, and options for them
static bool renditions_valid(int n, const int32_t* nrend, const void* opts) {
    if (n < 0 || (n > 0 && (!nrend || !opts))) return false;
    for (int i = 0; i < n; i++)
        if (nrend[i] < 1 || nrend[i] > H2J_MAX_RENDITIONS) return false;
    return true;
}

int64_t h2j_engine_submit_multi(h2j_engine* w, int n, const uint8_t* const* data, const size_t* sizes, const int32_t* nrend,
                                const h2j_out_opts2* opts, uint8_t* out, size_t out_cap, size_t* out_off, size_t* out_len,
                                int* status) {
    if (!w) return -1;
    if (!renditions_valid(n, nrend, opts)) return H2J_ERR_RENDITIONS;
    return submit_batch(w, n, data, sizes, nrend, h2j::multi_opts6(n, nrend, opts).data(), out, out_cap, out_off, out_len, status, false);
}

int64_t h2j_engine_submit_multi3(h2j_engine* w, int n, const uint8_t* const* data, const size_t* sizes, const int32_t* nrend,
                                 const h2j_out_opts3* opts, uint8_t* out, size_t out_cap, size_t* out_off, size_t* out_len,
                                 int* status) {
    if (!w) return -1;
    if (!renditions_valid(n, nrend, opts)) return H2J_ERR_RENDITIONS;
    return submit_batch(w, n, data, sizes, nrend, h2j::multi_opts6(n, nrend, opts).data(), out, out_cap, out_off, out_len, status, false);
}

int64_t h2j_engine_submit_multi5(h2j_engine* w, int n, const uint8_t* const* data, const size_t* sizes, const int32_t* nrend,
                                 const h2j_out_opts5* opts, uint8_t* out, size_t out_cap, size_t* out_off, size_t* out_len,
                                 int* status) {
    if (!w) return -1;
    if (!renditions_valid(n, nrend, opts)) return H2J_ERR_RENDITIONS;
    return submit_batch(w, n, data, sizes, nrend, h2j::multi_opts6(n, nrend, opts).data(), out, out_cap, out_off, out_len, status, false);
}

int64_t h2j_engine_submit_multi6(h2j_engine* w, int n, const uint8_t* const* data, const size_t* sizes, const int32_t* nrend,
                                 const h2j_out_opts6* opts, uint8_t* out, size_t out_cap, size_t* out_off, size_t* out_len,
                                 int* status, int32_t* out_wh) {
    if (!w) return -1;
    if (!renditions_valid(n, nrend, opts)) return H2J_ERR_RENDITIONS;
    return submit_batch(w, n, data, sizes, nrend, opts, out, out_cap, out_off, out_len, status, false, out_wh);
}

int h2j_engine_transcode_multi6(h2j_engine* w, int n, const uint8_t* const* data, const size_t* sizes, const int32_t* nrend,
                                const h2j_out_opts6* opts, uint8_t* out, size_t out_cap, size_t* out_off, size_t* out_len,
                                int* status, int32_t* out_wh) {
    if (!w) return -1;
    if (!renditions_valid(n, nrend, opts)) return H2J_ERR_RENDITIONS;
    const int64_t t = submit_batch(w, n, data, sizes, nrend, opts, out, out_cap, out_off, out_len, status, true, out_wh);
    return h2j_engine_wait(w, t);
}

int h2j_engine_transcode_multi(h2j_engine* w, int n, const uint8_t* const* data, const size_t* sizes, const int32_t* nrend,
                               const h2j_out_opts2* opts, uint8_t* out, size_t out_cap, size_t* out_off, size_t* out_len,
                               int* status) {
    if (!w) return -1;
    if (!renditions_valid(n, nrend, opts)) return H2J_ERR_RENDITIONS;
    const int64_t t = submit_batch(w, n, data, sizes, nrend, h2j::multi_opts6(n, nrend, opts).data(), out, out_cap, out_off, out_len, status, true);
    return h2j_engine_wait(w, t);
}

int h2j_engine_transcode_multi3(h2j_engine* w, int n, const uint8_t* const* data, const size_t* sizes, const int32_t* nrend,
                                const h2j_out_opts3* opts, uint8_t* out, size_t out_cap, size_t* out_off, size_t* out_len,
                                int* status) {
    if (!w) return -1;
    if (!renditions_valid(n, nrend, opts)) return H2J_ERR_RENDITIONS;
    const int64_t t = submit_batch(w, n, data, sizes, nrend, h2j::multi_opts6(n, nrend, opts).data(), out, out_cap, out_off, out_len, status, true);
    return h2j_engine_wait(w, t);
}

int h2j_engine_transcode_multi5(h2j_engine* w, int n, const uint8_t* const* data, const size_t* sizes, const int32_t* nrend,
                                const h2j_out_opts5* opts, uint8_t* out, size_t out_cap, size_t* out_off, size_t* out_len,
                                int* status) {
    if (!w) return -1;
    if (!renditions_valid(n, nrend, opts)) return H2J_ERR_RENDITIONS;
    const int64_t t = submit_batch(w, n, data, sizes, nrend, h2j::multi_opts6(n, nrend, opts).data(), out, out_cap, out_off, out_len, status, true);
    return h2j_engine_wait(w, t);
}

int64_t h2j_engine_submit_multi4(h2j_engine* w, int n, const uint8_t* const* data, const size_t* sizes, const int32_t* nrend,
                                 const h2j_out_opts4* opts, uint8_t* out, size_t out_cap, size_t* out_off, size_t* out_len,
                                 int* status) {
    if (!w) return -1;
    if (!renditions_valid(n, nrend, opts)) return H2J_ERR_RENDITIONS;
    return submit_batch(w, n, data, sizes, nrend, h2j::multi_opts6(n, nrend, opts).data(), out, out_cap, out_off, out_len, status, false);
}

int h2j_engine_transcode_multi4(h2j_engine* w, int n, const uint8_t* const* data, const size_t* sizes, const int32_t* nrend,
                                const h2j_out_opts4* opts, uint8_t* out, size_t out_cap, size_t* out_off, size_t* out_len,
                                int* status) {
    if (!w) return -1;
    if (!renditions_valid(n, nrend, opts)) return H2J_ERR_RENDITIONS;
    const int64_t t = submit_batch(w, n, data, sizes, nrend, h2j::multi_opts6(n, nrend, opts).data(), out, out_cap, out_off, out_len, status, true);
    return h2j_engine_wait(w, t);
}

int h2j_crop_window4(int w, int h, const h2j_out_opts4* o, int sei_orient, int32_t* win, int* ow, int* oh, int* orient) {
    if (!o) return H2J_ERR_OUT_OPTS;
    const h2j_out_opts6 o6 = h2j::opts6_of(*o);
    return h2j_crop_window6(w, h, &o6, sei_orient, win, ow, oh, orient);
}

int h2j_crop_window(int w, int h, const h2j_out_opts3* o, int32_t* win, int* ow, int* oh) {
    if (!o) return H2J_ERR_OUT_OPTS;
    const h2j_out_opts6 o6 = h2j::opts6_of(*o);
    int orient = 0;
    return h2j_crop_window6(w, h, &o6, 0, win, ow, oh, &orient);
}

int h2j_stream_orientation(const uint8_t* data, size_t size) {
    if (!data) return -1;
    const int codec = h2j::detect_codec(data, size);
    if (codec != 264 && codec != 265) return -100;
    return h2j::stream_display_orientation(data, size, codec);
}

int h2j_crop_window5(int w, int h, const h2j_out_opts5* o, int sei_orient, int32_t* win, int* ow, int* oh, int* orient) {
    if (!o) return H2J_ERR_OUT_OPTS;
    const h2j_out_opts6 o6 = h2j::opts6_of(*o);
    return h2j_crop_window6(w, h, &o6, sei_orient, win, ow, oh, orient);
}

int h2j_crop_window6(int w, int h, const h2j_out_opts6* o, int sei_orient, int32_t* win, int* ow, int* oh, int* orient) {
    if (!o || !win || !ow || !oh || !orient || w < 2 || h < 2 || w > 65536 || h > 65536 || ((w | h) & 1) || sei_orient < 0 ||
        sei_orient > 8 || !h2j::out_opts_valid(*o))
        return H2J_ERR_OUT_OPTS;
    const h2j::FrameJob::Output out = h2j::resolve_output(*o, w, h, sei_orient == 1 ? 0 : sei_orient);
    if (out.error) return out.error;
    *orient = out.orient;
    win[0] = out.win_x;
    win[1] = out.win_y;
    win[2] = out.win_w;
    win[3] = out.win_h;
    *ow = out.out_w();
    *oh = out.out_h();
    return 0;
}

int h2j_fit_size(int w, int h, int fit_w, int fit_h, int flags, int* ow, int* oh) {
    if (!ow || !oh || w < 2 || h < 2 || w > 65536 || h > 65536 || ((w | h) & 1) || !h2j::fit_valid(fit_w, fit_h, flags))
        return H2J_ERR_OUT_OPTS;
    const int64_t W = w, H = h;
    const int64_t bw = fit_w ? std::min<int64_t>(fit_w, W) : W, bh = fit_h ? std::min<int64_t>(fit_h, H) : H;
    int64_t wo, ho;
    if (flags & H2J_FIT_STRETCH) {
        wo = 2 * (bw / 2);
        ho = 2 * (bh / 2);
    } else if (bw * H <= bh * W) {  // the width binds
        wo = 2 * (bw / 2);
        ho = 2 * std::max<int64_t>(1, (H * wo) / (2 * W));
    } else {
        ho = 2 * (bh / 2);
        wo = 2 * std::max<int64_t>(1, (W * ho) / (2 * H));
    }
    *ow = static_cast<int>(wo);
    *oh = static_cast<int>(ho);
    return 0;
}

// parse one picture into jobs[0] of slot 0, with the outputs of its nrend option sets (valid ones)
static int single_job(h2j_engine* w, const uint8_t* data, size_t size, const h2j_out_opts6* o = &h2j::kPlainOutput, int nrend = 1) {
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
        if (rc[i] == 0) h2j::resolve_outputs(&h2j::kPlainOutput, 1, e.jobs[i]);
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

// the 8-bit planes K4 reads for one picture with output options o (h2j_engine_decode_scaled / _resized)
// (nrend renditions in flight, planes of rendition `pick`: h2j_engine_decode_multi)
// (info_n: entries of info the call has -- 4; 8: the window; 10: the orientation too; 12: qscale and sharpen too)
static int decode_jpeg_source(h2j_engine* w, const uint8_t* data, size_t size, const h2j_out_opts6* o, int nrend, int pick,
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
            e.fail(h2j::out_opts_message(o[r], e.jobs[0].hdr.out_w, e.jobs[0].hdr.out_h, e.jobs[0].sei_orient));
            return H2J_ERR_OUT_OPTS;
        }
    Slot& s = e.slot[0];
    // (12 entries: K4 runs too, for the quantiser scale it used)
    if (e.enqueue(s, info_n >= 12 ? 4 : 3, false) || e.sync(s)) return -3;
    // the picture K4 would read: the JPEG source view of the rendition
    const h2j_frame& f = s.plan.frames[0];
    const int vi = s.plan.rends[static_cast<size_t>(pick)].view;
    const h2j_scaled& sc = s.plan.scaled[vi];
    const h2j_frame v = s.plan.view(vi);
    const int w_ = v.out_w, h_ = v.out_h;
    int levels = 0;  // K3s levels among the views of the same window: two or more are K3p's
    for (int x = 0; x < s.plan.nv; x++)
        if (s.plan.scaled[x].scale_log2 >= 1 && s.plan.scaled[x].scale_log2 <= 3 && s.plan.vsrc[x] == s.plan.vsrc[vi])
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
    if (cap < static_cast<size_t>(w_) * h_ * 3 / 2) return e.fail("output buffer too small");
    const size_t pel = v.bit_depth > 8 ? 2 : 1;
    size_t bytes = 0;  // the view's planes in the arena, from v.pic2
    for (int c = 0; c < 3; c++) {
        // (an unscaled oriented view lies in the oriented planes, whose rows end with the oriented picture's)
        const int rows = (sc.scale_log2 || wo.sharpen) ? (h_ >> (c ? 1 : 0)) : wo.orient ? ((v.crop_y + h_) >> (c ? 1 : 0)) : (f.height >> (c ? 1 : 0));
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

int h2j_engine_decode_scaled(h2j_engine* w, const uint8_t* data, size_t size, int scale_log2, int max_dim,
                             uint8_t* planes_out, size_t cap, int* info) {
    const h2j_out_opts6 o = {scale_log2, max_dim, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, {0, 0, 0}};
    return decode_jpeg_source(w, data, size, &o, 1, 0, planes_out, cap, info);
}

int h2j_engine_decode_resized(h2j_engine* w, const uint8_t* data, size_t size, int fit_w, int fit_h, int flags,
                              uint8_t* planes_out, size_t cap, int* info) {
    const h2j_out_opts6 o = {0, 0, fit_w, fit_h, flags, 0, 0, 0, 0, 0, 0, 0, 0, {0, 0, 0}};
    return decode_jpeg_source(w, data, size, &o, 1, 0, planes_out, cap, info);
}

int h2j_engine_decode_multi(h2j_engine* w, const uint8_t* data, size_t size, int nrend, const h2j_out_opts2* opts, int pick,
                            uint8_t* planes_out, size_t cap, int* info) {
    if (nrend < 1 || nrend > H2J_MAX_RENDITIONS) return H2J_ERR_RENDITIONS;
    if (pick < 0 || pick >= nrend || !opts) return -1;
    return decode_jpeg_source(w, data, size, h2j::opts6_of(nrend, opts).data(), nrend, pick, planes_out, cap, info);
}

int h2j_engine_decode_multi3(h2j_engine* w, const uint8_t* data, size_t size, int nrend, const h2j_out_opts3* opts, int pick,
                             uint8_t* planes_out, size_t cap, int* info) {
    if (nrend < 1 || nrend > H2J_MAX_RENDITIONS) return H2J_ERR_RENDITIONS;
    if (pick < 0 || pick >= nrend || !opts) return -1;
    return decode_jpeg_source(w, data, size, h2j::opts6_of(nrend, opts).data(), nrend, pick, planes_out, cap, info, 8);
}

int h2j_engine_decode_multi5(h2j_engine* w, const uint8_t* data, size_t size, int nrend, const h2j_out_opts5* opts, int pick,
                             uint8_t* planes_out, size_t cap, int* info) {
    if (nrend < 1 || nrend > H2J_MAX_RENDITIONS) return H2J_ERR_RENDITIONS;
    if (pick < 0 || pick >= nrend || !opts) return -1;
    return decode_jpeg_source(w, data, size, h2j::opts6_of(nrend, opts).data(), nrend, pick, planes_out, cap, info, 12);
}

int h2j_engine_decode_multi4(h2j_engine* w, const uint8_t* data, size_t size, int nrend, const h2j_out_opts4* opts, int pick,
                             uint8_t* planes_out, size_t cap, int* info) {
    if (nrend < 1 || nrend > H2J_MAX_RENDITIONS) return H2J_ERR_RENDITIONS;
    if (pick < 0 || pick >= nrend || !opts) return -1;
    return decode_jpeg_source(w, data, size, h2j::opts6_of(nrend, opts).data(), nrend, pick, planes_out, cap, info, 10);
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
