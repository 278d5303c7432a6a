#include "bitstream.h"

#include <cstring>

namespace h2j {

// Both scans below look for a three-byte pattern that ends in a rare byte (01 / 03: one byte in 256 of
// entropy-coded data), so they search for that byte with memchr (the C library's vector scan) and look
// at the two bytes before a hit, where a byte-wise loop kept a zero count for every byte.
void split_annexb(const uint8_t* d, size_t n, std::vector<Nal>& out) {
    out.clear();
    long start = -1;
    auto close = [&](size_t e) {
        while (e > static_cast<size_t>(start) && d[e - 1] == 0) e--;
        out.push_back(Nal{d + start, e - static_cast<size_t>(start)});
    };
    // i: the first byte a start code may begin at (start codes do not overlap: after one, the
    // search goes on behind its 01)
    size_t i = 0;
    while (i + 2 < n) {
        const uint8_t* one = static_cast<const uint8_t*>(std::memchr(d + i + 2, 1, n - (i + 2)));
        if (!one) break;
        const size_t j = static_cast<size_t>(one - d);  // j - 2 >= i
        if (d[j - 1] == 0 && d[j - 2] == 0) {
            if (start >= 0) close(j - 2);
            i = j + 1;
            start = static_cast<long>(i);
        } else {
            i = j - 1;  // this 01 ends no start code; the next may begin at j - 1 at the earliest
        }
    }
    if (start >= 0 && static_cast<size_t>(start) < n) close(n);
}

size_t unescape_rbsp(const uint8_t* src, size_t n, uint8_t* dst) {
    // an emulation-prevention byte is a 03 after two zero bytes that lie behind the previous
    // removed one (the zero count restarts there): the stretches between them are copied whole
    size_t o = 0, seg = 0, from = 2;
    while (from < n) {
        const uint8_t* three = static_cast<const uint8_t*>(std::memchr(src + from, 3, n - from));
        if (!three) break;
        const size_t j = static_cast<size_t>(three - src);  // j - 2 >= seg
        if (src[j - 1] == 0 && src[j - 2] == 0) {
            std::memcpy(dst + o, src + seg, j - seg);
            o += j - seg;
            seg = j + 1;
            from = seg + 2;
        } else {
            from = j + 1;
        }
    }
    if (seg < n) {
        std::memcpy(dst + o, src + seg, n - seg);
        o += n - seg;
    }
    return o;
}

bool BitReader::more_rbsp_data() const {
    long last = static_cast<long>(n_) - 1;
    while (last >= 0 && p_[last] == 0) last--;
    if (last < 0) return false;
    int tz = 0;
    while (!((p_[last] >> tz) & 1)) tz++;
    size_t stop = static_cast<size_t>(last) * 8 + (7 - tz);
    return pos_ < stop;
}

int detect_codec(const uint8_t* d, size_t n) {
    std::vector<Nal> nals;
    split_annexb(d, n < (1u << 16) ? n : (1u << 16), nals);
    int hv = 0, hs = 0, hp = 0, as = 0, ap = 0;
    for (const Nal& nal : nals) {
        if (nal.n < 2) continue;
        uint8_t h0 = nal.p[0], h1 = nal.p[1];
        if (h0 & 0x80) continue;
        int t = (h0 >> 1) & 63, layer = ((h0 & 1) << 5) | (h1 >> 3), tid = h1 & 7;
        if (layer == 0 && tid >= 1) {
            if (t == 32) hv++;
            if (t == 33) hs++;
            if (t == 34) hp++;
        }
        int t4 = h0 & 31;
        if (t4 == 7) as++;
        if (t4 == 8) ap++;
    }
    if (hv && hs && hp) return 265;
    if (as && ap) return 264;
    return 0;
}

int sei_display_orientation(const uint8_t* rbsp, size_t n, bool hevc, int cur) {
    // [hor_flip][ver_flip][anticlockwise_rotation >> 14]: flip, then rotate anticlockwise, as an EXIF number
    static const uint8_t kCode[2][2][4] = {{{0, 8, 3, 6}, {4, 7, 2, 5}}, {{2, 5, 4, 7}, {3, 6, 0, 8}}};
    (void)hevc;  // the fields that differ (persistence / repetition period, extension) follow the ones read
    size_t pos = 0;
    while (n - pos >= 2) {  // a message has a type and a size byte at least; one byte left: the trailing bits
        uint32_t type = 0, size = 0;
        while (pos < n && rbsp[pos] == 0xFF && type < (1u << 20)) { type += 255; pos++; }
        if (pos >= n) break;
        type += rbsp[pos++];
        while (pos < n && rbsp[pos] == 0xFF && size < (1u << 20)) { size += 255; pos++; }
        if (pos >= n) {
            if (type == 47) cur = 0;
            break;
        }
        size += rbsp[pos++];
        if (size > n - pos) {  // runs past the NAL
            if (type == 47) cur = 0;
            break;
        }
        if (type == 47) {
            BitReader b(rbsp + pos, size);
            if (b.u(1)) {
                cur = 0;  // display_orientation_cancel_flag
            } else {
                const uint32_t hor = b.u(1), ver = b.u(1), rot = b.u(16);
                cur = (size < 3 || (rot & 0x3FFF)) ? 0 : kCode[hor][ver][rot >> 14];
            }
        }
        pos += size;
    }
    return cur;
}

int stream_display_orientation(const uint8_t* d, size_t n, int codec) {
    std::vector<Nal> nals;
    split_annexb(d, n, nals);
    std::vector<uint8_t> rbsp;
    int cur = 0;
    for (const Nal& nal : nals) {
        const size_t hdr = codec == 265 ? 2 : 1;
        if (nal.n < hdr) continue;
        const int type = codec == 265 ? (nal.p[0] >> 1) & 63 : nal.p[0] & 31;
        if (codec == 265 ? type == 39 : type == 6) {
            rbsp.resize(nal.n);
            const size_t rn = unescape_rbsp(nal.p + hdr, nal.n - hdr, rbsp.data());
            cur = sei_display_orientation(rbsp.data(), rn, codec == 265, cur);
        } else if (codec == 265) {
            // picture 0 starts at the first slice segment with first_slice_segment_in_pic_flag
            if (type <= 21 && !(type >= 10 && type <= 15) && nal.n > 2 && (nal.p[2] & 0x80)) break;
        } else if (type == 1 || type == 5) {
            break;
        }
    }
    return cur;
}

}  // namespace h2j
