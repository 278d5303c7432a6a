// Stand-alone driver of the HEIF demuxer (csrc/host/heif.cpp, linked alone): test infrastructure.
//   heif_host demux FILE             the demuxer's result as text: status, message, geometry, each tile's Annex-B
//                                    bytes in hex, and the file spans the payloads came from
//   heif_host probe FILE...          is_heif of each file, one 0 / 1 per line
//   heif_host corpus FILE OFF LEN    every truncation length of FILE, and every byte of FILE[OFF, OFF + LEN) set to
//                                    0x00, to 0xFF and incremented: each must end in an error with a message, or in a
//                                    result whose spans lie inside the buffer and whose tiles are in order.  Every
//                                    case runs on a heap copy of exactly its size, so a sanitizer build sees a read
//                                    past the end.  Prints the counts; exit 1 on a violated invariant
//   heif_host compose A B            heif_compose_orient(A, B)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "heif.h"

static bool read_file(const char* path, std::vector<uint8_t>& d) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    uint8_t buf[65536];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) d.insert(d.end(), buf, buf + n);
    std::fclose(f);
    return true;
}

// 0: an error with its message; 1: a sound result; -1: an invariant broken
static int check(const uint8_t* d, size_t n) {
    std::vector<uint8_t> copy(d, d + n);  // exactly n bytes on the heap
    h2j::HeifResult r;
    const int rc = h2j::is_heif(copy.data(), n) ? h2j::heif_demux(copy.data(), n, r) : -1;
    if (rc != 0) return (rc == -1 || (r.error == rc && r.message[0] && r.bytes.empty())) ? 0 : -1;
    for (const h2j::HeifSpan& s : r.spans)
        if (s.off > n || s.len > n - s.off) return -1;
    if (r.tile_off.size() != static_cast<size_t>(r.rows) * r.cols + 1 || r.tile_off[0] != 0 || r.tile_off.back() != r.bytes.size()) return -1;
    for (size_t t = 0; t + 1 < r.tile_off.size(); t++)
        if (r.tile_off[t] >= r.tile_off[t + 1]) return -1;
    if (r.orient < 0 || r.orient > 8 || r.orient == 1 || (r.codec != 264 && r.codec != 265)) return -1;
    return 1;
}

int main(int argc, char** argv) {
    if (argc >= 4 && !std::strcmp(argv[1], "compose")) {
        std::printf("%d\n", h2j::heif_compose_orient(std::atoi(argv[2]), std::atoi(argv[3])));
        return 0;
    }
    if (argc >= 3 && !std::strcmp(argv[1], "probe")) {
        for (int i = 2; i < argc; i++) {
            std::vector<uint8_t> d;
            if (!read_file(argv[i], d)) return 2;
            std::printf("%d\n", h2j::is_heif(d.data(), d.size()) ? 1 : 0);
        }
        return 0;
    }
    std::vector<uint8_t> d;
    if (argc < 3 || !read_file(argv[2], d)) {
        std::fprintf(stderr, "usage: heif_host demux FILE | probe FILE... | corpus FILE OFF LEN | compose A B\n");
        return 2;
    }
    if (!std::strcmp(argv[1], "demux")) {
        h2j::HeifResult r;
        const bool heif = h2j::is_heif(d.data(), d.size());
        const int rc = heif ? h2j::heif_demux(d.data(), d.size(), r) : 0;
        std::printf("heif %d\nstatus %d\nmessage %s\n", heif ? 1 : 0, rc, r.message);
        std::printf("codec %d grid %d rows %d cols %d w %d h %d orient %d\n", r.codec, r.grid ? 1 : 0, r.rows, r.cols, r.out_w, r.out_h, r.orient);
        for (size_t t = 0; t + 1 < r.tile_off.size(); t++) {
            std::printf("tile ");
            for (uint64_t i = r.tile_off[t]; i < r.tile_off[t + 1]; i++) std::printf("%02x", r.bytes[i]);
            std::printf("\n");
        }
        for (const h2j::HeifSpan& s : r.spans) std::printf("span %llu %llu\n", static_cast<unsigned long long>(s.off), static_cast<unsigned long long>(s.len));
        return 0;
    }
    if (!std::strcmp(argv[1], "corpus") && argc >= 5) {
        const size_t off = static_cast<size_t>(std::atoll(argv[3])), len = static_cast<size_t>(std::atoll(argv[4]));
        if (off > d.size() || len > d.size() - off) return 2;
        long cases = 0, errors = 0, sound = 0;
        auto tally = [&](int c, const char* what, size_t at) {
            cases++;
            if (c < 0) {
                std::printf("invariant broken: %s at %zu\n", what, at);
                std::exit(1);
            }
            (c ? sound : errors)++;
        };
        for (size_t n = 0; n < d.size(); n++) tally(check(d.data(), n), "truncation", n);
        std::vector<uint8_t> m(d);
        for (size_t i = off; i < off + len; i++) {
            const uint8_t keep = m[i];
            const uint8_t vals[3] = {0x00, 0xFF, static_cast<uint8_t>(keep + 1)};
            for (uint8_t v : vals) {
                m[i] = v;
                tally(check(m.data(), m.size()), "mutation", i);
            }
            m[i] = keep;
        }
        std::printf("cases %ld errors %ld sound %ld\n", cases, errors, sound);
        return 0;
    }
    return 2;
}
