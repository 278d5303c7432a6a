// HEIF / HEIC input: a pure demuxer from an ISO-BMFF `meta` box to Annex-B streams.
//
// Reads the primary item of a HEIF file (ISO/IEC 23008-12 over ISO/IEC 14496-12 boxes): a single
// `hvc1` or `avc1` item, or a `grid` of `hvc1` tile items, and rewrites the decoder configuration
// (hvcC / avcC parameter sets) and the length-prefixed NAL units of each item as an Annex-B stream.
// The entropy decoders then run on those streams (heif_parse.cpp).  No threads, no GPU call, nothing
// of the engine: <cstdint> and <vector> only (and <cstddef> for size_t).  The bytes are untrusted: every size, offset, count and
// index is checked against the buffer before it is used, and nothing is allocated by an unchecked field.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace h2j {

// a part of the file an item's bytes were read from (what the robustness tests bound)
struct HeifSpan {
    uint64_t off, len;
};

struct HeifResult {
    int error = 0;      // 0, or the negative status below
    char message[128];  // the error's text ("" without one)
    int codec = 0;      // 265 / 264
    bool grid = false;  // a grid of rows x cols tiles whose output is out_w x out_h
    int rows = 1, cols = 1, out_w = 0, out_h = 0;
    int orient = 0;     // irot / imir of the primary item as an orientation 0, 2..8 (include/h2j.h)
    // the `nclx` colr property of the primary item (a grid without one: the first its tiles carry): colour_primaries,
    // transfer_characteristics, matrix_coefficients, full_range_flag.  rICC / prof profiles are ignored
    bool nclx = false;
    int colour[4] = {2, 2, 2, 0};
    // the Annex-B streams, one per tile in raster order (a single item: one), back to back:
    // stream t is bytes[tile_off[t] .. tile_off[t + 1])
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> tile_off;
    std::vector<HeifSpan> spans;  // where in the file the payloads came from
    HeifResult() { message[0] = 0; }
};

// statuses of a HEIF input that fails (the parsers' own keep theirs)
enum {
    H2J_HEIF_MALFORMED = -110,    // truncated or malformed box structure
    H2J_HEIF_NO_PRIMARY = -111,   // no primary item
    H2J_HEIF_UNSUPPORTED = -112,  // item type, essential property, construction method, grid of AVC tiles
    H2J_HEIF_NO_CONFIG = -113,    // item has no decoder configuration
    H2J_HEIF_DATA = -114,         // item data outside the file
    H2J_HEIF_GRID = -115,         // grid descriptor and references disagree
};

// bytes 4..7 are `ftyp`, the box is 16..4096 bytes and a multiple of 4, and the major or a compatible
// brand is one of heic heix hevc hevx mif1 msf1 avci.  Anything else is not HEIF input.
bool is_heif(const uint8_t* d, size_t n);

// The primary item of a HEIF file as Annex-B streams.  Returns r.error.
int heif_demux(const uint8_t* d, size_t n, HeifResult& r);

// The orientation (0, 2..8) of `then` applied to a picture already oriented by `first` (either 0..8)
int heif_compose_orient(int first, int then);

}  // namespace h2j
