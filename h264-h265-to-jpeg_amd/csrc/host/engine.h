// The batch engine's types (internal: engine.cpp runs the pipeline, engine_api.cpp is the C ABI of include/h2j.h).
#pragma once
#include <algorithm>
#include <chrono>
#include <deque>
#include <memory>
#include <string>

#include "affinity.h"
#include "chunk_plan.h"  // and include/h2j*.h, job.h
#include "thread_pool.h"  // and the standard headers it includes

namespace h2j {

inline double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// a device buffer / a pinned host buffer that grows by half; growing frees the old block (its contents are not kept)
template <typename P, void* (*Alloc)(size_t), int (*Free)(void*)>
struct GrowBuf {
    P* p = nullptr;
    size_t cap = 0;
    bool ensure(size_t n) {
        if (n <= cap) return true;
        if (p) Free(p);
        cap = std::max(n, cap + cap / 2);
        p = static_cast<P*>(Alloc(cap));
        if (!p) cap = 0;
        return p != nullptr;
    }
    void release() {
        if (p) Free(p);
        p = nullptr;
        cap = 0;
    }
};
typedef GrowBuf<void, h2j_gpu_malloc, h2j_gpu_free> DevBuf;
typedef GrowBuf<uint8_t, h2j_gpu_host_alloc, h2j_gpu_host_free> HostBuf;

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
    EV_SCALE,       // after K3o (oriented output), K3s / K3r / K3p (scaled output), K3v (colour), K3u (finishing), K3b (padded output) and K3c (RGB output)
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
       ST_H2D_BYTES, ST_PAY_COPIED, ST_SCALE, ST_RENDITIONS, ST_PARSED, ST_RAW_BYTES, ST_PAD_BYTES, ST_COLOUR_BYTES, ST_N };  // ST_PACK: host time packing records into staging; ST_SCALE: K3o + K3s + K3r + K3p + K3v + K3u + K3b + K3c
// ST_RAW_BYTES: bytes of the raw (RGB) renditions delivered; K3c's time counts in ST_SCALE
// ST_PAD_BYTES: canvas bytes K3b wrote for the padded renditions; K3b's time counts in ST_SCALE
// ST_COLOUR_BYTES: plane bytes K3v wrote for the colour-converted renditions; K3v's time counts in ST_SCALE
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
    std::vector<h2j_out_opts8> opts;           // output options per rendition, item-major (a plain item has one rendition)
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
    // one optional late stage of launch (K3o, K3u, K3b, K3c): nothing in a chunk without records for it; fn null: the
    // kernel library has no such stage
    template <typename Rec, int NCLS>
    int late_stage(Slot& s, const StageMap<Rec, NCLS>& m,
                   int (*fn)(const h2j_gpu_batch*, const Rec*, const int32_t*, const int32_t*, const int32_t*, void*), const char* missing);
    int enqueue_payload_copy(Slot& s);
    // Wait for slot s and copy its payloads down (entropy chunks).
    int sync(Slot& s);
};

int parse_any(const uint8_t* d, size_t n, FrameJob& job);
// the outputs of a parsed job: every rendition's is resolved on its own (out_opts.h), and invalid options or a
// stage the kernel library lacks (H2J_ERR_NO_STAGE) fail that rendition alone
void resolve_outputs(const h2j_out_opts8* o, int nr, FrameJob& job);
// the message of an output that failed with H2J_ERR_NO_STAGE: the stage the kernel library lacks
const char* no_stage_message(const FrameJob::Output& o);
std::vector<int> chunk_bounds(int n);             // the synchronous plan: a shrinking tail
std::vector<int> chunk_bounds_throughput(int n);  // asynchronous batches
constexpr double kSlotHbmBudget = 64e9;  // at most, per slot (two slots per engine)

}  // namespace h2j
