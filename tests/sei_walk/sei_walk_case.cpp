// The SEI walker over malformed input, as a stand-alone program for a sanitizer build (tests/test_orient_sei_walk.py
// compiles it with -fsanitize=address,undefined beside bitstream.cpp): every buffer is a heap block of exactly its
// size, so a read past the NAL is a report.  Prints the number of inputs walked and a digest of the results.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bitstream.h"

namespace {

uint32_t rng_state = 20261020u;
uint32_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 17;
    rng_state ^= rng_state << 5;
    return rng_state;
}

uint64_t digest = 1469598103934665603ull;
long walked = 0;

void walk(const std::vector<uint8_t>& v) {
    uint8_t* p = new uint8_t[v.size() ? v.size() : 1];  // exactly the bytes: no slack behind them
    if (!v.empty()) std::memcpy(p, v.data(), v.size());
    for (int hevc = 0; hevc < 2; hevc++)
        for (int cur : {0, 6}) {
            const int r = h2j::sei_display_orientation(p, v.size(), hevc != 0, cur);
            if (r < 0 || r > 8 || r == 1) {
                std::printf("orientation %d out of range\n", r);
                std::exit(1);
            }
            digest = (digest ^ static_cast<uint64_t>(r)) * 1099511628211ull;
        }
    delete[] p;
    walked++;
}

void walk_stream(const std::vector<uint8_t>& v) {
    uint8_t* p = new uint8_t[v.size() ? v.size() : 1];
    if (!v.empty()) std::memcpy(p, v.data(), v.size());
    for (int codec : {264, 265}) {
        const int r = h2j::stream_display_orientation(p, v.size(), codec);
        if (r < 0 || r > 8 || r == 1) {
            std::printf("orientation %d out of range\n", r);
            std::exit(1);
        }
        digest = (digest ^ static_cast<uint64_t>(r)) * 1099511628211ull;
    }
    delete[] p;
    walked++;
}

}  // namespace

int main() {
    // every string of up to 4 bytes over the bytes that steer the walk
    const uint8_t alpha[] = {0x00, 0x01, 0x02, 0x03, 0x2F, 0x80, 0xFF, 0x10};
    for (int len = 0; len <= 4; len++) {
        long n = 1;
        for (int i = 0; i < len; i++) n *= 8;
        for (long k = 0; k < n; k++) {
            std::vector<uint8_t> v;
            long q = k;
            for (int i = 0; i < len; i++, q /= 8) v.push_back(alpha[q % 8]);
            walk(v);
        }
    }
    // a valid message (type 47, 3 bytes: no flip, one quarter turn) cut at every length, with every size byte
    const uint8_t msg[] = {47, 3, 0x08, 0x00, 0x18, 0x80};
    for (size_t len = 0; len <= sizeof(msg); len++)
        for (int size = 0; size < 256; size++) {
            std::vector<uint8_t> v(msg, msg + len);
            if (len > 1) v[1] = static_cast<uint8_t>(size);
            walk(v);
        }
    // seeded random strings biased to 0xFF runs, type 47 and small sizes
    for (int it = 0; it < 200000; it++) {
        std::vector<uint8_t> v(rnd() % 48);
        for (uint8_t& b : v) {
            const uint32_t r = rnd();
            b = (r & 7) == 0 ? 0xFF : (r & 7) == 1 ? 47 : (r & 7) == 2 ? static_cast<uint8_t>((r >> 8) & 7) : static_cast<uint8_t>(r >> 8);
        }
        walk(v);
    }
    // whole streams: start codes, SEI and slice NAL headers of both codecs in random order, random payloads
    const uint8_t heads[] = {0x06, 0x4E, 0x01, 0x26, 0x65, 0x40, 0x67, 0x42};
    for (int it = 0; it < 20000; it++) {
        std::vector<uint8_t> v;
        for (int nal = rnd() % 6; nal > 0; nal--) {
            for (int z = rnd() % 3; z > 0; z--) v.push_back(0);
            v.insert(v.end(), {0, 0, 1});
            if (rnd() % 8) v.push_back(heads[rnd() % 8]);
            if (rnd() % 4) v.push_back(static_cast<uint8_t>(rnd() % 3 ? 0x01 : rnd()));
            for (int n = rnd() % 12; n > 0; n--) v.push_back(static_cast<uint8_t>(rnd() % 3 ? rnd() : (rnd() % 2 ? 47 : 0xFF)));
        }
        walk_stream(v);
    }
    std::printf("walked %ld digest %016llx\n", walked, static_cast<unsigned long long>(digest));
    return 0;
}
