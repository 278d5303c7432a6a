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
#include "engine.h"

#include <cmath>
#include <cstdlib>
#include <cstring>

#include "bitstream.h"
#include "heif.h"
#include "jpeg_writer.h"
#include "out_opts.h"

// The kernel library's optional late stages, null when the library in use is older than them (weak references:
// bound when this library loads, so a stand-in or an older build selected beside it still loads): K3o; K3u and the
// K4 entry that takes the quantiser scale from the caller; K3c; K3b; K3v
extern "C" int h2j_gpu_orient(const h2j_gpu_batch*, const h2j_orient*, const int32_t*, const int32_t*, const int32_t*, void*)
    __attribute__((weak));
extern "C" int h2j_gpu_finish(const h2j_gpu_batch*, const h2j_finish*, const int32_t*, const int32_t*, const int32_t*, void*)
    __attribute__((weak));
extern "C" int h2j_gpu_jpeg2(const h2j_gpu_batch*, const int32_t*, void*) __attribute__((weak));
extern "C" int h2j_gpu_rgb(const h2j_gpu_batch*, const h2j_rgb*, const int32_t*, const int32_t*, const int32_t*, void*)
    __attribute__((weak));
extern "C" int h2j_gpu_pad(const h2j_gpu_batch*, const h2j_pad*, const int32_t*, const int32_t*, const int32_t*, void*)
    __attribute__((weak));
extern "C" int h2j_gpu_colour(const h2j_gpu_batch*, const h2j_colour*, const int32_t*, const int32_t*, const int32_t*, void*)
    __attribute__((weak));

namespace h2j {

int parse_any(const uint8_t* d, size_t n, FrameJob& job) {
    // a job slot is reused from batch to batch: what an earlier HEIF input left in it goes before anything is parsed
    if (job.demuxed.capacity()) std::vector<uint8_t>().swap(job.demuxed);
    if (is_heif(d, n)) return heif_parse_picture(d, n, job);  // its items as Annex-B streams, then the parsers below
    const int codec = detect_codec(d, n);
    if (codec == 265) return hevc_parse_picture(d, n, job);
    if (codec == 264) return h264_parse_picture(d, n, job);
    job.clear();
    job.error = -100;
    job.message = "not an H.264/H.265 Annex-B stream";
    return -100;
}

template <typename Rec, int NCLS>
int Engine::late_stage(Slot& s, const StageMap<Rec, NCLS>& m,
                       int (*fn)(const h2j_gpu_batch*, const Rec*, const int32_t*, const int32_t*, const int32_t*, void*), const char* missing) {
    if (s.stages < 3 || m.empty()) return 0;
    if (!fn) return drain_fail(s, missing);
    const Rec* map = reinterpret_cast<const Rec*>(static_cast<const uint8_t*>(s.d_in.p) + m.at);
    return fn(&s.batch, map, m.first, m.count, m.tiles, s.stream) ? drain_fail(s, h2j_gpu_last_error()) : 0;
}

// The optional stages, in the order they are checked and reported, each described once: whether the kernel library
// has the stage (its weak entry points), which outputs need it, what an output that needs a missing one is told, and
// the stage's launch on a slot
struct OptionalStage {
    bool (*present)();
    bool (*needed)(const FrameJob::Output&);
    const char* missing;
    int (*launch)(Engine&, Slot&);
};
enum { STAGE_ORIENT, STAGE_COLOUR, STAGE_FINISH, STAGE_RGB, STAGE_PAD };  // (checked and reported in this order: orient, colour, finish: the launch order)
const OptionalStage kStages[] = {
    {[] { return h2j_gpu_orient != nullptr; }, [](const FrameJob::Output& o) { return o.orient != 0; },
     "the kernel library has no orientation stage (h2j_gpu_orient): oriented output needs a newer libh2j_hip.so",
     [](Engine& e, Slot& s) { return e.late_stage(s, s.plan.orientmap, h2j_gpu_orient, kStages[STAGE_ORIENT].missing); }},
    {[] { return h2j_gpu_colour != nullptr; }, [](const FrameJob::Output& o) { return o.colour != 0; },
     "the kernel library has no colour stage (h2j_gpu_colour): colour-converted output needs a newer libh2j_hip.so",
     [](Engine& e, Slot& s) { return e.late_stage(s, s.plan.colmap, h2j_gpu_colour, kStages[STAGE_COLOUR].missing); }},
    {[] { return h2j_gpu_finish && h2j_gpu_jpeg2; }, [](const FrameJob::Output& o) { return o.qscale != 0 || o.sharpen != 0; },
     "the kernel library has no finishing stage (h2j_gpu_finish, h2j_gpu_jpeg2): qscale and sharpen need a newer libh2j_hip.so",
     [](Engine& e, Slot& s) { return e.late_stage(s, s.plan.finmap, h2j_gpu_finish, kStages[STAGE_FINISH].missing); }},
    {[] { return h2j_gpu_rgb != nullptr; }, [](const FrameJob::Output& o) { return o.format != 0; },
     "the kernel library has no RGB stage (h2j_gpu_rgb): raw output needs a newer libh2j_hip.so",
     [](Engine& e, Slot& s) { return e.late_stage(s, s.plan.rgbmap, h2j_gpu_rgb, kStages[STAGE_RGB].missing); }},
    {[] { return h2j_gpu_pad != nullptr; }, [](const FrameJob::Output& o) { return o.pad != 0; },
     "the kernel library has no padding stage (h2j_gpu_pad): padded output needs a newer libh2j_hip.so",
     [](Engine& e, Slot& s) { return e.late_stage(s, s.plan.padmap, h2j_gpu_pad, kStages[STAGE_PAD].missing); }},
};

const char* no_stage_message(const FrameJob::Output& o) {
    for (const OptionalStage& st : kStages)
        if (st.needed(o) && !st.present()) return st.missing;
    return kStages[STAGE_RGB].missing;  // (asked of an output that lacks no stage: the last one's, as it always was)
}
void resolve_outputs(const h2j_out_opts8* o, int nr, FrameJob& job) {
    job.nouts = nr;
    for (int r = 0; r < nr; r++) {
        job.outs[r] = FrameJob::Output();
        if (out_opts_valid(o[r])) job.outs[r] = resolve_output(o[r], job.hdr.out_w, job.hdr.out_h, job.sei_orient, job.colour);
        else job.outs[r].error = H2J_ERR_OUT_OPTS;
        for (const OptionalStage& st : kStages)
            if (job.outs[r].error == 0 && st.needed(job.outs[r]) && !st.present()) job.outs[r].error = H2J_ERR_NO_STAGE;
    }
}
// parse one item of a batch with the output options of its nr renditions (a plain item: one).  The item
// is not parsed when none is valid: it fails with the first one's message.  *ran: the entropy decode ran
static int parse_item_multi(const uint8_t* d, size_t n, const h2j_out_opts8* o, int nr, FrameJob& job, bool* ran) {
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
    }
    put(p.orientmap.at, p.orientmap.map.data(), p.orientmap.bytes());  // the late stages' maps: nothing in chunks without
    put(p.finmap.at, p.finmap.map.data(), p.finmap.bytes());
    put(p.rgbmap.at, p.rgbmap.map.data(), p.rgbmap.bytes());
    put(p.padmap.at, p.padmap.map.data(), p.padmap.bytes());
    put(p.colmap.at, p.colmap.map.data(), p.colmap.bytes());
    if (p.qforced && !p.compact()) put(p.at.qforce, p.vqscale.data(), static_cast<size_t>(p.nv) * 4);
    if (p.compact()) {  // the views K4 / K5 run on, and their forced scales, packed
        h2j_frame* jc = reinterpret_cast<h2j_frame*>(hin + p.at.jcompact);
        int32_t* qf = reinterpret_cast<int32_t*>(hin + p.at.qforce);
        for (size_t i = 0; i < p.jviews.size(); i++) {
            jc[i] = p.view(p.jviews[i]);
            if (p.qforced) qf[i] = p.vqscale[p.jviews[i]];
        }
    }
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
    // the late stages run only in chunks with records for them (which exist only when the kernel library has the stage):
    // K3o in front of the scale stage, K3u, K3b and K3c (out of place: K4 reads what it read, or the canvas K3b made)
    // behind it
    if (kStages[STAGE_ORIENT].launch(*this, s)) return -1;
    if (s.stages >= 3 && h2j_gpu_scale(&b, st)) return drain_fail(s, h2j_gpu_last_error());  // K3s, K3r: no launch without scaled pictures
    if (kStages[STAGE_COLOUR].launch(*this, s)) return -1;  // K3v: in front of K3u, which sharpens the converted planes
    if (kStages[STAGE_FINISH].launch(*this, s) || kStages[STAGE_PAD].launch(*this, s) || kStages[STAGE_RGB].launch(*this, s)) return -1;
    h2j_gpu_event_record(s.ev[EV_SCALE], st);
    // a chunk of raw renditions only: nobody asked for a JPEG, so no K4 / K5 and no payload (the pool's byte count,
    // which K5 would have written, is cleared instead)
    const bool jpegs = p.njpeg > 0;
    // K4: through h2j_gpu_jpeg2 only in chunks with a forced quantiser scale (likewise)
    if (s.stages >= 4 && jpegs && p.qforced) {
        if (!h2j_gpu_jpeg2 || h2j_gpu_jpeg2(&jb, reinterpret_cast<const int32_t*>(static_cast<const uint8_t*>(s.d_in.p) + p.at.qforce), st))
            return drain_fail(s, h2j_gpu_jpeg2 ? h2j_gpu_last_error() : kStages[STAGE_FINISH].missing);
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
    if (s.stages >= 3) stats[ST_PAD_BYTES] += static_cast<double>(s.plan.pad_bytes);
    if (s.stages >= 3) stats[ST_COLOUR_BYTES] += static_cast<double>(s.plan.colour_bytes);
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
        if (j.outs[r].error == 0 && j.outs[r].format) est += 3.0 * j.outs[r].canvas_w() * j.outs[r].canvas_h() + 4096;
    // padded outputs: the canvas is one more view -- its 8-bit planes, jcoef / tile region and share of the payload
    // pool, from the canvas size (one that shares a canvas with another rendition: an overestimate)
    for (int r = 0; r < j.nouts; r++)
        if (j.outs[r].error == 0 && j.outs[r].pad) est += 14.5 * j.outs[r].box_w * j.outs[r].box_h + 8192;
    // converted outputs: the 8-bit planes K3v writes (one that shares them with another rendition: an overestimate)
    for (int r = 0; r < j.nouts; r++)
        if (j.outs[r].error == 0 && j.outs[r].colour) est += 1.5 * (j.outs[r].out_w() + 15.0) * j.outs[r].out_h() + 1024;
    return est;
}
// JPEG outputs of a job (at least one: the chunk bound counts a failed item as one; a padded output is two views)
static int views_estimate(const FrameJob& j) {
    int n = j.nouts;
    for (int r = 0; r < j.nouts; r++) n += (j.outs[r].error == 0 && j.outs[r].pad) ? 1 : 0;
    return std::max(1, n);
}

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
                    else if (b->status[o] == H2J_ERR_OUT_OPTS) b->msg[o] = out_opts_message(b->opts[static_cast<size_t>(o)], (*jobs)[i].hdr.out_w, (*jobs)[i].hdr.out_h, (*jobs)[i].sei_orient, (*jobs)[i].colour);
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
                        b.out_wh[2 * o] = jo.canvas_w();
                        b.out_wh[2 * o + 1] = jo.canvas_h();
                    }
                    // a raw rendition's size is known here: one that cannot fit the output buffer behind the raw
                    // renditions planned before it (JPEGs only take more) fails now, and K3c does not run for it
                    if (jo.error == 0 && jo.format) {
                        const size_t len = 3 * static_cast<size_t>(jo.canvas_w()) * jo.canvas_h();
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
