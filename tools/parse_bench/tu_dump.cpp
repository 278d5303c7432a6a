// Dumps what the host parser hands K0 for one picture, as plain little-endian binary (tests/k0_ref.py reads it):
//   "K0TU", then 11 int32: codec, width, height, bit_depth, bit_depth_c, log2ctb, scaling_list, rext, ntu, ncoef,
//   nsl; then ntu h2j_tu records (16 B), ncoef h2j_coef entries (4 B, h2j_tu.coef indexes them), nsl bytes of
//   scaling factors (FrameJob::sl).
// usage: tu_dump in.h265 out.bin [in out ...]   (exit 1 at the first stream the parser refuses)
// Built like parse_bench:
//   g++ -O2 -std=c++11 -pthread -I../../include -I../../h264-h265-to-jpeg_amd/csrc/host tu_dump.cpp \
//       ../../h264-h265-to-jpeg_amd/csrc/host/{bitstream,cabac_tables,hevc_parser,h264_parser}.cpp
#include <cstdio>
#include <vector>

#include "bitstream.h"
#include "job.h"

int main(int argc, char** argv) {
    if (argc < 3 || (argc & 1) == 0) {
        std::fprintf(stderr, "usage: tu_dump in out [in out ...]\n");
        return 2;
    }
    h2j::FrameJob job;
    for (int i = 1; i + 1 < argc; i += 2) {
        FILE* f = std::fopen(argv[i], "rb");
        if (!f) {
            std::fprintf(stderr, "%s: cannot open\n", argv[i]);
            return 1;
        }
        std::vector<uint8_t> s;
        uint8_t buf[65536];
        size_t n;
        while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) s.insert(s.end(), buf, buf + n);
        std::fclose(f);
        const int codec = h2j::detect_codec(s.data(), s.size());
        const int rc = codec == 265 ? h2j::hevc_parse_picture(s.data(), s.size(), job) : h2j::h264_parse_picture(s.data(), s.size(), job);
        if (rc) {
            std::fprintf(stderr, "%s: parse error %d: %s\n", argv[i], rc, job.message.c_str());
            return 1;
        }
        const h2j_frame& h = job.hdr;
        const h2j_coef* co = job.coefs.data() + h.coef;
        const size_t nco = job.coefs.size() - h.coef;
        const int32_t head[11] = {h.codec, h.width, h.height, h.bit_depth, h.bit_depth_c, h.log2ctb, h.scaling_list, h.rext,
                                  static_cast<int32_t>(job.tus.size()), static_cast<int32_t>(nco), static_cast<int32_t>(job.sl.size())};
        FILE* o = std::fopen(argv[i + 1], "wb");
        if (!o) {
            std::fprintf(stderr, "%s: cannot write\n", argv[i + 1]);
            return 1;
        }
        std::fwrite("K0TU", 1, 4, o);
        std::fwrite(head, sizeof(head), 1, o);
        std::fwrite(job.tus.data(), sizeof(h2j_tu), job.tus.size(), o);
        std::fwrite(co, sizeof(h2j_coef), nco, o);
        std::fwrite(job.sl.data(), 1, job.sl.size(), o);
        std::fclose(o);
    }
    return 0;
}
