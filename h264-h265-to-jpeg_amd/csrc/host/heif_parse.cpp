// HEIF input to job records: the demuxer (heif.cpp) in front of the entropy decoders.
#include "bitstream.h"
#include "heif.h"
#include "job.h"

namespace h2j {

int heif_parse_picture(const uint8_t* data, size_t size, FrameJob& job) {
    HeifResult r;
    if (heif_demux(data, size, r)) {
        job.clear();
        job.error = r.error;
        job.message = r.message;
        return r.error;
    }
    job.demuxed.swap(r.bytes);
    const uint8_t* base = job.demuxed.data();
    int rc;
    if (r.grid) {
        const size_t T = r.tile_off.size() - 1;
        std::vector<const uint8_t*> tiles(T);
        std::vector<size_t> sizes(T);
        for (size_t t = 0; t < T; t++) {
            tiles[t] = base + r.tile_off[t];
            sizes[t] = static_cast<size_t>(r.tile_off[t + 1] - r.tile_off[t]);
        }
        rc = hevc_parse_grid(tiles.data(), sizes.data(), r.rows, r.cols, r.out_w, r.out_h, job);
    } else {
        rc = r.codec == 265 ? hevc_parse_picture(base, job.demuxed.size(), job) : h264_parse_picture(base, job.demuxed.size(), job);
    }
    // the file's transform properties say how to show the picture; a display orientation SEI inside the item
    // stands only where the file has none (a grid's tiles' SEI messages are never read)
    if (rc == 0 && r.orient) job.sei_orient = r.orient;
    return rc;
}

int heif_orientation(const uint8_t* data, size_t size) {
    HeifResult r;
    if (heif_demux(data, size, r)) return r.error;
    if (r.orient || r.grid) return r.orient;
    return stream_display_orientation(r.bytes.data(), r.bytes.size(), r.codec);
}

}  // namespace h2j
