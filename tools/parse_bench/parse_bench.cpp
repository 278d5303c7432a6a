// Host-only timing of the entropy decoders (no GPU): parses every stream of
// the argument list `reps` times on T threads (each with its own FrameJob,
// streams dealt round-robin) and prints ms/frame (wall / frames, and per
// thread) and TUs/frame.
//   g++ -O2 -std=c++11 -pthread -I../../include -I../../h264-h265-to-jpeg_amd/csrc/host parse_bench.cpp \
//       ../../h264-h265-to-jpeg_amd/csrc/host/{bitstream,cabac_tables,hevc_parser,h264_parser}.cpp
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>
#include <vector>

#include "bitstream.h"
#include "cabac.h"
#include "job.h"
#ifdef H2J_HEIF_INPUT
#include "heif.h"
#endif
#ifdef H2J_SAMPLE
#include "sampler.h"
#endif

#ifdef H2J_CABAC_COUNT
#ifdef __linux__
#include <linux/perf_event.h>
#include <sys/syscall.h>
#include <unistd.h>
#include <cerrno>
#include <cstring>
#endif
namespace h2j {
thread_local unsigned long long g_bins_ctx = 0, g_bins_byp = 0;
thread_local ResidualStats g_rstat = {};
thread_local BranchSiteStat g_bsite[BS_COUNT] = {};
}
namespace {
// -b: a hardware counter of this thread (user mode), or -1 where the kernel does not allow one
int perf_open(unsigned long long config) {
#ifdef __linux__
    perf_event_attr pe;
    std::memset(&pe, 0, sizeof(pe));
    pe.type = PERF_TYPE_HARDWARE;
    pe.size = sizeof(pe);
    pe.config = config;
    pe.exclude_kernel = 1;
    pe.exclude_hv = 1;
    return static_cast<int>(syscall(SYS_perf_event_open, &pe, 0, -1, -1, 0));
#else
    (void)config;
    return -1;
#endif
}
unsigned long long perf_read(int fd) {
    unsigned long long v = 0;
#ifdef __linux__
    if (fd < 0 || read(fd, &v, sizeof(v)) != static_cast<ssize_t>(sizeof(v))) v = 0;
#endif
    return v;
}
}  // namespace
#endif

// FNV-1a over one picture's records (summed over pictures: an order-independent checksum)
static unsigned long long job_digest(const h2j::FrameJob& job) {
    unsigned long long hsh = 1469598103934665603ull;
    auto mix = [&](const void* p, size_t n) {
        const unsigned char* q = static_cast<const unsigned char*>(p);
        for (size_t j = 0; j < n; j++) hsh = (hsh ^ q[j]) * 1099511628211ull;
    };
    mix(job.tus.data(), job.tus.size() * sizeof(h2j_tu));
    mix(job.coefs.data(), job.coefs.size() * sizeof(h2j_coef));
    mix(job.ctbs.data(), job.ctbs.size() * sizeof(h2j_ctb));
    mix(job.slices.data(), job.slices.size() * sizeof(h2j_slice));
    mix(&job.hdr, sizeof(job.hdr));
    return hsh;
}

int main(int argc, char** argv) {
#ifdef H2J_SAMPLE
    h2j_sample::start();
#endif
    if (argc < 2) {
        std::fprintf(stderr, "usage: parse_bench file... [-r reps] [-t threads] [-d (output digest)] [-m] [-s] [-p n] [-b (residual breakdown)] [-B (branch sites)]\n");
        return 2;
    }
    int reps = 3, threads = 1, pthreads = 1;
    bool want_digest = false, want_hist = false, want_min = false, want_breakdown = false, want_sites = false;
    std::vector<std::vector<uint8_t>> streams;
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        if (a == "-r" && i + 1 < argc) {
            reps = std::atoi(argv[++i]);
            continue;
        }
        if (a == "-d") {
            want_digest = true;
            continue;
        }
        if (a == "-b") {  // residual-syntax breakdown (-DH2J_CABAC_COUNT builds)
            want_breakdown = true;
            continue;
        }
        if (a == "-B") {  // branch-site table of the slice-data path (-DH2J_CABAC_COUNT builds)
            want_sites = true;
            continue;
        }
        if (a == "-m") {  // min-of-reps per stream (robust to a noisy host): sum of per-stream minima
            want_min = true;
            continue;
        }
        if (a == "-s") {  // transform-block histogram by (component, size, cbf)
            want_hist = true;
            continue;
        }
        if (a == "-p" && i + 1 < argc) {  // threads inside one picture (independent slices)
            pthreads = std::atoi(argv[++i]);
            continue;
        }
        if (a == "-t" && i + 1 < argc) {
            threads = std::atoi(argv[++i]);
            continue;
        }
        FILE* f = std::fopen(argv[i], "rb");
        if (!f) continue;
        std::vector<uint8_t> d;
        uint8_t buf[65536];
        size_t n;
        while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) d.insert(d.end(), buf, buf + n);
        std::fclose(f);
        streams.push_back(d);
    }
    if (want_breakdown) {
#ifdef H2J_CABAC_COUNT
        // what HEVC residual_coding is fed, per picture and in total over the streams given (one pass on
        // this thread), the sub-blocks / transform blocks that took each special path of
        // HevcParser::residual(), and the parse's cycles and branch misses where the kernel allows counters
        const int fc = perf_open(PERF_COUNT_HW_CPU_CYCLES), fb = perf_open(PERF_COUNT_HW_BRANCH_MISSES);
        const int perf_errno = fc < 0 ? errno : 0;
        h2j::FrameJob job;
        unsigned long long digest = 0;
        const unsigned long long c0 = perf_read(fc), b0 = perf_read(fb);
        for (const auto& s : streams) {
            const int codec = h2j::detect_codec(s.data(), s.size());
            const int rc = codec == 265 ? h2j::hevc_parse_picture(s.data(), s.size(), job)
                                        : h2j::h264_parse_picture(s.data(), s.size(), job);
            if (rc) {
                std::fprintf(stderr, "parse error %d: %s\n", rc, job.message.c_str());
                return 1;
            }
            digest += job_digest(job);
        }
        const unsigned long long cyc = perf_read(fc) - c0, brm = perf_read(fb) - b0;
        const h2j::ResidualStats& r = h2j::g_rstat;
        const double nf = static_cast<double>(streams.size());
        std::printf("breakdown of %zu pictures, digest %016llx\n", streams.size(), digest);
        std::printf("%-44s %14s %14s\n", "item", "per picture", "total");
        auto row = [&](const char* name, unsigned long long v) { std::printf("%-44s %14.0f %14llu\n", name, v / nf, v); };
        row("context_bins", h2j::g_bins_ctx);
        row("bypass_bins", h2j::g_bins_byp);
        row("tbs_with_residual", r.tbs);
        row("sub_blocks_visited", r.sb_visited);
        row("coded_sub_block_flag_bins", r.csbf_bins);
        row("coded_sub_blocks", r.sb_coded);
        row("sig_coeff_flag_bins_pos_gt0", r.sig_bins);
        row("sig_coeff_flag_bins_pos0", r.sig0_bins);
        row("greater1_bins", r.gt1_bins);
        row("greater2_bins", r.gt2_bins);
        row("last_sig_coeff_prefix_bins", r.last_bins);
        row("coefficients", r.coefs);
        row("coded_sub_blocks_1_coef", r.sb_by_coefs[0]);
        row("coded_sub_blocks_2_coefs", r.sb_by_coefs[1]);
        row("coded_sub_blocks_3_coefs", r.sb_by_coefs[2]);
        row("coded_sub_blocks_4_7_coefs", r.sb_by_coefs[3]);
        row("coded_sub_blocks_8plus_coefs", r.sb_by_coefs[4]);
        row("coefs_with_abs_level_remaining", r.rem_coefs);
        row("sub_blocks_with_abs_level_remaining", r.rem_sbs);
        row("sign_batch_sub_blocks", r.sign_batch_sbs);
        row("sign_single_sub_blocks", r.sign_single_sbs);
        row("path_one_coef", r.one_coef);
        row("path_one_coef_escape", r.one_coef_esc);
        row("path_one_coef_escape_persistent_rice", r.one_coef_esc_price);
        row("path_one_coef_transform_skip", r.one_coef_tskip);
        row("path_one_coef_transquant_bypass", r.one_coef_bypass);
        row("path_one_coef_escape_transform_skip", r.one_coef_esc_tskip);
        row("path_one_coef_escape_transquant_bypass", r.one_coef_esc_bypass);
        row("path_dc_only_last_sub_block", r.dc_last_sb);
        row("path_dc_only_tb", r.dc_only_tb);
        row("path_sign_pair_single_steps", r.sign_pair);
        if (fc >= 0 && fb >= 0)
            std::printf("perf: %.0f cycles, %.0f branch misses per picture; %.2f cycles per bin, %.2f misses per coded sub-block\n",
                        cyc / nf, brm / nf, cyc / static_cast<double>(h2j::g_bins_ctx + h2j::g_bins_byp),
                        r.sb_coded ? brm / static_cast<double>(r.sb_coded) : 0.0);
        else
            std::printf("perf: hardware counters not available here (perf_event_open: %s); skipped\n", std::strerror(perf_errno));
        return 0;
#else
        std::fprintf(stderr, "-b needs a -DH2J_CABAC_COUNT build\n");
        return 2;
#endif
    }
    if (want_sites) {
#if defined(H2J_CABAC_COUNT) && !defined(H2J_NO_BRANCH_SITES)
        // every data-dependent branch of the HEVC slice-data path as a named site (cabac.h): how often it
        // ran, how often its condition held, and the misses of a two-bit predictor simulated per site --
        // the same on every machine, so the table ranks the sites; one pass over the streams on this thread
        static const char* const kSite[h2j::BS_COUNT] = {
#define H2J_X(n) #n,
            H2J_BRANCH_SITES(H2J_X)
#undef H2J_X
        };
        h2j::FrameJob job;
        unsigned long long digest = 0;
        for (const auto& s : streams) {
            const int codec = h2j::detect_codec(s.data(), s.size());
            const int rc = codec == 265 ? h2j::hevc_parse_picture(s.data(), s.size(), job)
                                        : h2j::h264_parse_picture(s.data(), s.size(), job);
            if (rc) {
                std::fprintf(stderr, "parse error %d: %s\n", rc, job.message.c_str());
                return 1;
            }
            digest += job_digest(job);
        }
        const double nf = static_cast<double>(streams.size());
        std::printf("branch sites of %zu pictures, digest %016llx\n", streams.size(), digest);
        std::printf("%-22s %14s %14s %14s %12s\n", "site", "executed", "taken", "sim_misses", "misses/pic");
        unsigned long long te = 0, tt = 0, tm = 0;
        for (int k = 0; k < h2j::BS_COUNT; k++) {
            const h2j::BranchSiteStat& b = h2j::g_bsite[k];
            std::printf("%-22s %14llu %14llu %14llu %12.0f\n", kSite[k], b.exec, b.taken, b.miss, b.miss / nf);
            te += b.exec;
            tt += b.taken;
            tm += b.miss;
        }
        std::printf("%-22s %14llu %14llu %14llu %12.0f\n", "all_sites", te, tt, tm, tm / nf);
        return 0;
#else
        std::fprintf(stderr, "-B needs a -DH2J_CABAC_COUNT build (without -DH2J_NO_BRANCH_SITES)\n");
        return 2;
#endif
    }
    if (want_min) {
        h2j::FrameJob job;
        double sum = 0;
        for (const auto& s : streams) {
            double best = 1e30;
            for (int r = 0; r < reps; r++) {
                const auto t0 = std::chrono::steady_clock::now();
                const int codec = h2j::detect_codec(s.data(), s.size());
                const int rc = codec == 265 ? h2j::hevc_parse_picture(s.data(), s.size(), job)
                                            : h2j::h264_parse_picture(s.data(), s.size(), job);
                const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
                if (rc) return 1;
                best = std::min(best, ms);
            }
            sum += best;
        }
        std::printf("min-of-%d: %.4f ms/frame\n", reps, sum / static_cast<double>(streams.size()));
        return 0;
    }
    const int total = reps * static_cast<int>(streams.size());
    std::atomic<int> next(0), failed(0);
    std::atomic<size_t> tus(0), coefs(0), bytes(0);
    std::atomic<unsigned long long> bins_ctx(0), bins_byp(0);
    std::atomic<unsigned long long> digest(0);  // order-independent checksum of all parse outputs
    std::atomic<unsigned long long> hist[2][4][2];
    for (auto& a : hist) for (auto& b : a) for (auto& c : b) c = 0;
    auto worker = [&]() {
        h2j::FrameJob job;
        job.threads = pthreads;
        size_t t = 0, c = 0, b = 0;
        for (int i = next++; i < total; i = next++) {
            const auto& s = streams[i % streams.size()];
            const int codec = h2j::detect_codec(s.data(), s.size());
#ifdef H2J_HEIF_INPUT  // built with heif.cpp and heif_parse.cpp: HEIF files parse as the engine parses them
            const int rc = h2j::is_heif(s.data(), s.size()) ? h2j::heif_parse_picture(s.data(), s.size(), job)
                           : codec == 265                   ? h2j::hevc_parse_picture(s.data(), s.size(), job)
                                                            : h2j::h264_parse_picture(s.data(), s.size(), job);
#else
            const int rc = codec == 265 ? h2j::hevc_parse_picture(s.data(), s.size(), job)
                                        : h2j::h264_parse_picture(s.data(), s.size(), job);
#endif
            if (rc) {
                std::fprintf(stderr, "parse error %d: %s\n", rc, job.message.c_str());
                failed++;
                return;
            }
            t += job.tus.size();
            if (want_hist)
                for (const h2j_tu& u : job.tus)
                    if (u.log2n >= 2 && u.log2n <= 5) hist[u.c ? 1 : 0][u.log2n - 2][(u.flags & H2J_TU_CBF) ? 1 : 0]++;
            c += job.coefs.size();
            b += s.size();
            if (!want_digest) continue;
            digest += job_digest(job);
        }
        tus += t;
        coefs += c;
        bytes += b;
#ifdef H2J_CABAC_COUNT
        bins_ctx += h2j::g_bins_ctx;
        bins_byp += h2j::g_bins_byp;
#endif
    };
    auto t0 = std::chrono::steady_clock::now();
    std::vector<std::thread> pool;
    // one thread: parse on the main thread (the -DH2J_SAMPLE process timer signals the main thread)
    if (threads == 1) worker();
    else
        for (int k = 0; k < threads; k++) pool.emplace_back(worker);
    for (auto& th : pool) th.join();
    if (failed) return 1;
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    const double nf = total;
    std::printf("%d thr: %.3f ms/frame wall, %.3f ms/frame/thread  %.0f TUs/frame  %.0f coefs/frame  %.1f MB/s  digest %016llx\n",
                threads, ms / nf, ms * threads / nf, tus / nf, coefs / nf, bytes / (ms / 1e3) / 1e6,
                static_cast<unsigned long long>(digest));
    if (want_hist)
        for (int c = 0; c < 2; c++)
            for (int l = 0; l < 4; l++)
                std::printf("%s %2dx%-2d: %8.0f TBs/frame, %8.0f with residual\n", c ? "chroma" : "luma  ", 4 << l, 4 << l,
                            (hist[c][l][0] + hist[c][l][1]) / nf, hist[c][l][1] / nf);
    if (bins_ctx + bins_byp)
        std::printf("bins/frame: %.0f context-coded, %.0f bypass; %.2f ns per bin\n", bins_ctx / nf, bins_byp / nf,
                    ms * 1e6 * threads / static_cast<double>(bins_ctx + bins_byp));
    return 0;
}
