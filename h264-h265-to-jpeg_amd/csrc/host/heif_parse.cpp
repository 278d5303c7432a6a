// HEIF input to job records: the demuxer (heif.cpp) in front of the entropy decoders.
#include <algorithm>

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
    // likewise the file's nclx colour property wins over the VUI of the item's SPS
    if (rc == 0 && r.nclx) std::copy(r.colour, r.colour + 4, job.colour);
    return rc;
}

int heif_stream_colour(const uint8_t* data, size_t size, int* colour) {
    HeifResult r;
    if (heif_demux(data, size, r)) return r.error;
    if (r.nclx) {
        std::copy(r.colour, r.colour + 4, colour);
        return 0;
    }
    // (a grid: tile 0's stream -- the tiles' parameter sets are equal)
    const size_t n0 = r.tile_off.size() > 1 ? static_cast<size_t>(r.tile_off[1] - r.tile_off[0]) : r.bytes.size();
    const bool ok = r.codec == 265 ? hevc_stream_colour(r.bytes.data(), n0, colour) : h264_stream_colour(r.bytes.data(), n0, colour);
    return ok ? 0 : -100;
}

int heif_orientation(const uint8_t* data, size_t size) {
    HeifResult r;
    if (heif_demux(data, size, r)) return r.error;
    if (r.orient || r.grid) return r.orient;
    return stream_display_orientation(r.bytes.data(), r.bytes.size(), r.codec);
}

}  // namespace h2j
