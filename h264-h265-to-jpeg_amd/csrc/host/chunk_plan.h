// The plan of one GPU chunk: everything the engine decides about a set of parsed pictures before it
// touches a buffer -- frames and views, the arena layout, the workgroup maps, the staging layout and the
// scalar fields of the batch descriptor.  Pure host arithmetic on the job records: no GPU call.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "h2j_gpu.h"
#include "job.h"

namespace h2j {

// H.264 pictures with more MB rows than this are reconstructed by several K1 workgroups
constexpr int kK1BandRows = 68;

// upper bound of one block's entropy-coded size (code lengths <= 16, values <= 16 bits)
constexpr size_t kSegBytesPerBlock = 272;

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// The map of a late stage (K3o, K3v, K3u, K3b, K3c; include/h2j_gpu.h h2j_gpu_orient, h2j_gpu_colour, h2j_gpu_finish, h2j_gpu_pad,
// h2j_gpu_rgb): the stage's
// records grouped by class, uploaded behind the other maps, with each class's first record, count and the most
// workgroups one record of the class needs -- one launch per class present.  A chunk without the stage has an empty
// map, uploads nothing for it and does not launch it
template <typename Rec, int NCLS>
struct StageMap {
    std::vector<Rec> map;
    int32_t first[NCLS] = {0}, count[NCLS] = {0}, tiles[NCLS] = {0};
    size_t at = 0;  // the map's byte offset in the staging buffer
    void clear() {
        map.clear();
        for (int cls = 0; cls < NCLS; cls++) first[cls] = count[cls] = tiles[cls] = 0;
    }
    bool empty() const { return map.empty(); }
    size_t bytes() const { return map.size() * sizeof(Rec); }
    size_t staging_bytes() const { return empty() ? 0 : bytes() + 16; }  // nothing: the offsets behind it are what they were
    // the records in class order, their own order inside a class
    template <typename ClassOf, typename TilesOf>
    void group(const std::vector<Rec>& records, ClassOf class_of, TilesOf tiles_of) {
        for (int cls = 0; cls < NCLS && !records.empty(); cls++) {
            first[cls] = static_cast<int32_t>(map.size());
            for (const Rec& rec : records) {
                if (class_of(rec) != cls) continue;
                map.push_back(rec);
                count[cls]++;
                tiles[cls] = std::max<int32_t>(tiles[cls], tiles_of(rec));
            }
        }
    }
};

struct ChunkPlan {
    // Frames and views: nf frames (decoded pictures) and nv >= nf JPEG source views, frame-major.  A view
    // is (frame, window, resolved output, qscale, sharpen) with its own h2j_scaled, scaled planes, jcoef / tile region and jstat;
    // the first view of a frame -- its unscaled rendition if it has one -- keeps the frame's own jcoef
    // and jstat.  One rendition per item: nv == nf, view k is frame k
    int nf = 0, nv = 0;
    std::vector<h2j_frame> frames;   // per frame: the job's header with its record ranges and arena offsets
    std::vector<h2j_scaled> scaled;  // per view: its JPEG size and, for a scaled output, its scaled planes
    std::vector<uint64_t> vjcoef;    // per view: its jcoef / tile region
    std::vector<int> vfirst;         // per frame: its first view (nf + 1 entries)
    struct Rend {
        int out, view;  // index in the batch's output arrays; the view that holds its JPEG
        int rgb;        // -1: the JPEG; else the raw output (rgbs) that holds its pixels
    };
    std::vector<Rend> rends;  // the chunk's renditions (those with valid options), frame-major

    // Windows (crop and cover): a distinct (frame, window) pair is uploaded as a copy of the frame behind the
    // nf frames, with the window added to its conformance crop (wframe), so that K3s, K3r and K3p read "the
    // cropped planes of pic2" of the copy with the code they have; K0 .. K3 walk the nf frames only.  An
    // unscaled windowed view needs no kernel: K4 reads the frame in place through the view (view()).
    // A chunk without windows has none of this and uploads what it always did
    struct Window {
        int frame, x, y, w, h;  // the frame, and the window in luma samples of its cropped picture
        int osrc;               // -1, or the oriented source (orients) the window lies in, in its coordinates
    };
    std::vector<Window> wins;  // the chunk's distinct windows, frame-major
    std::vector<int> vsrc;     // per view: the index the scale kernels find its source under -- its frame, or
                               // nf + its window; views of one source with K3s levels form one pyramid
    std::vector<int> fstat;    // per frame: the jstat slot (of njstat) that is the frame's own -- its first
                               // view's, or one behind the views' when that view is an unscaled window (the
                               // frame's jstat takes K3 SAO's variance sum of the whole picture and the
                               // device-side error flags; the window's sum is K4a's, in the view's own)
    int njstat = 0;            // jstat slots: nv, and one more per such frame
    h2j_frame wframe(int j) const;  // the frame copy of window j

    // Orientation (K3o): a distinct (frame, orientation) pair is an oriented source -- the frame's cropped
    // planes, rotated or mirrored by K3o into an arena region of their own (opic; rows of whole 64-byte groups,
    // planes on 64-byte boundaries, the frame's sample type).  Every output of an oriented picture is a window
    // of it (the whole picture is the window 0, 0, W, H): its frame copy has pic == pic2 == opic, no
    // conformance crop and the oriented strides, so K3s, K3r, K3p and K4 read it with the code they have.
    // A chunk without oriented outputs has none of this and uploads what it always did
    std::vector<h2j_orient> orients;                      // the chunk's oriented sources, frame-major
    StageMap<h2j_orient, H2J_ORIENT_CLASSES> orientmap;  // the same grouped by class (sample type x transposing)

    // Finishing (K3u, forced qscale): a view is (frame, window, resolved output, qscale, sharpen).  Views that differ
    // only in qscale or sharpen share nothing: each has its scaled planes and runs the scale stage for itself (of
    // two views at one K3s level of a pyramid, K3p writes the first and K3s the others).  A sharpened view has a
    // record: K3u reads what the view would be without sharpening (base_view) and writes 8-bit planes of its own
    // (upic; the spic strides), which view() then shows with pic == pic2.  The views' forced scales are uploaded
    // (one int32 a view) only by chunks that force one.  A chunk without finishing has none of this and uploads
    // what it always did
    std::vector<int32_t> vqscale;    // per view: the quantiser scale K4b is to use, 0: the rate control's
    std::vector<int> vsharpen;       // per view: the unsharp mask's strength, 0: none
    std::vector<int> vfin;           // per view: -1, or its record in fins
    std::vector<h2j_finish> fins;    // the chunk's sharpened outputs, view-major
    StageMap<h2j_finish, H2J_FINISH_CLASSES> finmap;  // the same grouped by source class
    bool qforced = false;            // a view of the chunk forces its quantiser scale
    h2j_frame base_view(int v) const;  // view v without its sharpening: what K3u reads (a converted view: K3v's planes)

    // RGB output (K3c): a rendition has a format; a raw one (RGB pixels instead of a file) is served by a view like any
    // other -- the view of a JPEG rendition of the same frame with its (window, resolved output, sharpen) if there is
    // one (the quantiser scale does not change the planes), else one of its own -- and has a record: K3c reads what
    // view() shows K4 and writes the pixels into an arena region behind upic (256-byte aligned start per output, tight
    // rows).  Renditions of one view with one layout share a record.  The region is what the chunk copies to the host
    // beside the JPEG payloads.  A chunk without raw outputs has none of this and uploads what it always did
    std::vector<h2j_rgb> rgbs;    // the chunk's raw outputs, view-major
    std::vector<int> rgbview;     // per raw output: its view
    StageMap<h2j_rgb, H2J_RGB_CLASSES> rgbmap;  // the same grouped by source class
    size_t rgb_base = 0, rgb_bytes = 0;  // the region: arena offset, bytes (whole 256-byte groups)
    std::vector<char> vjpeg;      // per view: a JPEG rendition shows it (else raw ones only: its JPEG is never assembled)
    int njpeg = 0;                // such views; 0: a chunk of raw renditions only, which runs no K4 / K5
    // K4 / K5 run on the views some JPEG rendition shows.  Where that is not all of them (0 < njpeg < nv) those views
    // are uploaded once more as an array of their own (jviews: their indices, in view order), which K4 / K5 take as
    // their pictures, and the forced scales are packed for them: a view that only raw renditions show gets no JPEG,
    // no payload in the pool and no share of the payload estimate
    std::vector<int> jviews;
    bool compact() const { return njpeg > 0 && njpeg < nv; }

    // Padded output (K3b): a padded rendition has two views.  The view of its picture part is a view like any other,
    // found the way a raw output finds its view (the quantiser scale does not change the planes), so an unpadded
    // rendition with the same (window, resolved output, sharpen) shares it and the scale stage and K3u run once; padded
    // renditions alone never set its vjpeg.  The canvas view is what K4 / K5 or K3c read: a view of its own (vpad: its
    // record; vsrc -1, scale_log2 0, no sharpening of its own; jpeg_w x jpeg_h the canvas) whose planes K3b writes into
    // an arena region behind upic (bpic; the spic strides), which view() shows with pic == pic2.  Renditions with one
    // picture view, one canvas size, one place, one fill colour -- and one quantiser scale, unless raw -- share a canvas
    // view.  A chunk without padded outputs has none of this and uploads what it always did
    std::vector<int> vpad;         // per view: -1, or its record in pads (a canvas view)
    std::vector<h2j_pad> pads;     // the chunk's canvases, view-major
    std::vector<int> padview, padsrc;  // per canvas: its view, the view of its picture part
    StageMap<h2j_pad, H2J_PAD_CLASSES> padmap;  // the same grouped by source class
    size_t pad_bytes = 0;          // the canvas bytes K3b writes (their planes' rows with the row padding)

    // Colour (K3v): a view is (frame, window, resolved output, qscale, sharpen, resolved colour).  A converted view has a
    // record: K3v reads what the view would be without the option and without sharpening (scaled_view: the scale
    // stage's planes, or the frame, window or oriented source) and writes 8-bit planes of its own (vpic; the spic
    // strides), which base_view() then shows with pic == pic2 -- so K3u, K3b, K3c and K4 see a wide source.  Converted
    // views of one frame with one (source, resolved output, colour) -- they differ in qscale or sharpen -- share one
    // record (vcol names it); a converted scaled view whose planes an earlier view of the frame has (the same source
    // and output, converted or not) reads that view's (vshare) and is left out of the scale stage.  A chunk without
    // converted outputs has none of this and uploads what it always did
    std::vector<int> vcolour;       // per view: 0, or the resolved colour (FrameJob::Output::colour)
    std::vector<int> vcol;          // per view: -1, or its record in cols
    std::vector<int> vshare;        // per view: -1, or the earlier view whose scaled planes it reads
    std::vector<h2j_colour> cols;   // the chunk's converted outputs, view-major
    std::vector<int> colview;       // per converted output: the first view that shows it
    StageMap<h2j_colour, H2J_COLOUR_CLASSES> colmap;  // the same grouped by class (2 x source class + work class)
    size_t colour_bytes = 0;        // the plane bytes K3v writes (rows with the row padding)
    h2j_frame scaled_view(int v) const;  // view v without colour and sharpening: what K3v reads

    // arena layout: [zeroed: maps + CTB TU ranges + jstat][pic][pic2][spic][opic][vpic][upic][bpic][rgb][jcoef][res][aux]
    size_t arena_bytes = 0, zero_bytes = 0, jstat_base = 0, jstat_stride = 0;
    size_t seg_cap = 0;  // payload pool bytes (K5)
    int tiles = 0;       // 256-block tiles of the largest view (K5's tile_bits scratch: nv x tiles)
    double px = 0;       // JPEG pixels of the chunk (payload estimate)

    // workgroup maps (include/h2j_gpu.h h2j_gpu_batch), uploaded behind the records
    std::vector<uint32_t> k1map, k1map8, k1all, k1hevc, saomap;
    std::vector<h2j_scaled> scalemap;
    std::vector<h2j_pyramid> pyrmap;
    bool views = false;  // a views array is uploaded (a scaled picture, or several renditions of a frame)

    // staging layout: byte offset of each array in the one buffer the chunk uploads
    struct Staging {
        size_t frames = 0, tus = 0, coefs = 0, ctbs = 0, slices = 0, sl = 0, k1map = 0, k1all = 0, sao = 0, k1map8 = 0,
               k1hevc = 0, jframes = 0, scale = 0, pyr = 0, qforce = 0, jcompact = 0, bytes = 0;
    } at;  // (the late stages' maps: StageMap::at)

    // the descriptor's scalar fields (counts, maxima, codec / sample-type masks, classes); its pointers,
    // jpeg_dense and seg_cap are the engine's to fill once it has the buffers
    h2j_gpu_batch desc{};

    // the JPEG source view of view v: what K4 (variance, FDCT) and K5 read as "the picture"
    h2j_frame view(int v) const;

    // an empty plan of nf frames; the vectors keep their capacity from chunk to chunk
    void reset(int nframes);
};

// Plan the chunk of jobs[live[0..]] (parsed jobs, each with at least one valid output: every frame has a view) into p; p's vectors are
// reused from chunk to chunk.
void plan_chunk(const std::vector<FrameJob>& jobs, const std::vector<int>& live, ChunkPlan& p);

}  // namespace h2j
