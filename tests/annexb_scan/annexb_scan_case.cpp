// The Annex-B scan (bitstream.cpp split_annexb, unescape_rbsp) as a stand-alone program, for tests/test_annexb_scan.py:
// it is run as built and again built with -fsanitize=address,undefined.  The argument is a file of cases, each a
// little-endian 32-bit length and that many bytes.  Every case is copied into a heap block of exactly its size and
// the output goes into a block of exactly the input's size, so a read or write past either is a sanitizer report.
// Per case one line: the number of NAL units, "offset,length" of each, the CRC-32 of the whole buffer after
// emulation-prevention removal, and the CRC-32 of all NAL payloads after it, back to back.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "bitstream.h"

namespace {

uint32_t crc32(uint32_t crc, const uint8_t* p, size_t n) {
    crc = ~crc;
    for (size_t i = 0; i < n; i++) {
        crc ^= p[i];
        for (int k = 0; k < 8; k++) crc = (crc >> 1) ^ (0xEDB88320u & (0u - (crc & 1u)));
    }
    return ~crc;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: annexb_scan_case cases.bin\n");
        return 2;
    }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    long cases = 0;
    for (;;) {
        uint8_t lb[4];
        if (std::fread(lb, 1, 4, f) != 4) break;
        const size_t n = lb[0] | (lb[1] << 8) | (lb[2] << 16) | (static_cast<size_t>(lb[3]) << 24);
        uint8_t* d = new uint8_t[n ? n : 1];
        uint8_t* o = new uint8_t[n ? n : 1];
        if (n && std::fread(d, 1, n, f) != n) return 2;
        std::vector<h2j::Nal> nals;
        h2j::split_annexb(d, n, nals);
        std::printf("%zu", nals.size());
        uint32_t crc_nals = 0;
        for (const h2j::Nal& nal : nals) {
            std::printf(" %td,%zu", nal.p - d, nal.n);
            if (nal.p < d || nal.n > n || static_cast<size_t>(nal.p - d) > n - nal.n) {
                std::printf(" out of bounds\n");
                return 1;
            }
            const size_t rn = h2j::unescape_rbsp(nal.p, nal.n, o);
            crc_nals = crc32(crc_nals, o, rn);
        }
        const size_t wn = h2j::unescape_rbsp(d, n, o);
        std::printf(" %zu %08x %08x\n", wn, crc32(0, o, wn), crc_nals);
        delete[] d;
        delete[] o;
        cases++;
    }
    std::fclose(f);
    std::fprintf(stderr, "%ld cases\n", cases);
    return 0;
}
