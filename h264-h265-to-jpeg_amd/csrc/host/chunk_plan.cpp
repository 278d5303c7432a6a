#include "chunk_plan.h"

#include <algorithm>
#include <cstring>
#include <utility>

namespace h2j {
namespace {

// 256-byte aligned regions handed out front to back (the arena, the staging buffer)
struct Cursor {
    size_t off = 0;
    size_t take(size_t bytes) {
        const size_t at = off;
        off = align_up(off + bytes, 256);
        return at;
    }
};

// (key, value) pairs -> their values appended to out, smallest key first, equal keys in their order;
// sorts e in place, so a caller can walk it afterwards in map order
typedef std::vector<std::pair<long long, uint32_t>> Keyed;
void append_by_key(Keyed& e, std::vector<uint32_t>& out) {
    std::stable_sort(e.begin(), e.end(),
                     [](const Keyed::value_type& a, const Keyed::value_type& b) { return a.first < b.first; });
    for (const auto& x : e) out.push_back(x.second);
}

bool k3s_level(const h2j_scaled& sc) { return sc.scale_log2 >= 1 && sc.scale_log2 <= 3; }
size_t view_blocks(const h2j_scaled& sc) { return static_cast<size_t>(((sc.jpeg_w + 15) >> 4) * ((sc.jpeg_h + 15) >> 4)) * 6; }
bool banded(const h2j_frame& f) { return f.codec == H2J_CODEC_H264 && f.k1bands > 1; }

// Number the frames' records, and give every frame its views: one per distinct (window, output) of its
// renditions, the unscaled whole picture first.  A view's JPEG size is the cropped picture's, its scaled size or
// its fit size (K4 / K5 work on that picture)
void number_frames_and_views(const std::vector<FrameJob>& jobs, const std::vector<int>& live, ChunkPlan& p) {
    size_t ntu = 0, ncoef = 0, nctb = 0, nslice = 0, nsl = 0;
    h2j_gpu_batch& d = p.desc;
    for (int k = 0; k < p.nf; k++) {
        const FrameJob& j = jobs[live[k]];
        d.max_ntu = std::max(d.max_ntu, static_cast<int>(j.tus.size()));
        h2j_frame& f = p.frames[k];
        f = j.hdr;
        f.tu = static_cast<uint32_t>(ntu);
        f.ntu = static_cast<uint32_t>(j.tus.size());
        f.coef = static_cast<uint32_t>(ncoef);
        f.ctb = static_cast<uint32_t>(nctb);
        f.slice = static_cast<uint32_t>(nslice);
        f.nslice = static_cast<uint32_t>(j.slices.size());
        f.sl = static_cast<uint32_t>(nsl);
        ntu += j.tus.size();
        ncoef += j.coefs.size();
        nctb += j.ctbs.size();
        nslice += j.slices.size();
        nsl += j.sl.size();
        // H.264 K1: pictures taller than 1080p run on one workgroup per 16 MB rows
        // (a single 16-wave workgroup would walk 5+ rows per wave)
        // (MBAFF frames run on one workgroup: their K1 / deblocking walk macroblock pairs)
        f.k1bands = (f.codec == H2J_CODEC_H264 && f.ctb_h > kK1BandRows && !f.mbaff) ? (f.ctb_h + 15) / 16 : 1;
        f.xline = 0;
        const size_t v0 = p.scaled.size(), w0 = p.wins.size(), o0 = p.orients.size();
        p.vfirst[k] = static_cast<int>(v0);
        // the frame, or nf + the frame's window, added if new; an oriented output's window (the whole oriented
        // picture is one) lies in the frame's oriented source of that orientation, added if new
        auto source_of = [&](const FrameJob::Output& o) {
            if (!o.windowed && !o.orient) return k;
            int osrc = -1;
            for (size_t i = o0; o.orient && i < p.orients.size(); i++)
                if (p.orients[i].orient == o.orient) osrc = static_cast<int>(i);
            if (o.orient && osrc < 0) {
                h2j_orient rec{};
                rec.frame = k;
                rec.orient = o.orient;
                p.orients.push_back(rec);
                osrc = static_cast<int>(p.orients.size()) - 1;
            }
            for (size_t w = w0; w < p.wins.size(); w++)
                if (p.wins[w].osrc == osrc && p.wins[w].x == o.win_x && p.wins[w].y == o.win_y && p.wins[w].w == o.win_w &&
                    p.wins[w].h == o.win_h)
                    return p.nf + static_cast<int>(w);
            p.wins.push_back(ChunkPlan::Window{k, o.win_x, o.win_y, o.win_w, o.win_h, osrc});
            return p.nf + static_cast<int>(p.wins.size()) - 1;
        };
        auto view_of = [&](const FrameJob::Output& o) {  // the frame's view with this window and output, added if new
            const int src = source_of(o);
            for (size_t v = v0; v < p.scaled.size(); v++) {
                const h2j_scaled& sv = p.scaled[v];
                // (a raw output reads any view with its planes: the quantiser scale does not change them; so does the
                // canvas of a padded output.  A canvas view has the source -1: it is nobody's picture)
                if (p.vsrc[v] == src && sv.scale_log2 == o.scale_log2 && (p.vqscale[v] == o.qscale || o.format || o.pad) && p.vsharpen[v] == o.sharpen &&
                    p.vcolour[v] == o.colour && (o.scale_log2 != H2J_SCALE_RESAMPLE || (sv.jpeg_w == o.fit_w && sv.jpeg_h == o.fit_h)))
                    return static_cast<int>(v);
            }
            h2j_scaled sc{};
            sc.frame = k;
            sc.scale_log2 = o.scale_log2;
            const bool resample = sc.scale_log2 == H2J_SCALE_RESAMPLE;
            sc.jpeg_w = resample ? o.fit_w : h2j_scaled_dim((o.windowed || o.orient) ? o.win_w : f.out_w, sc.scale_log2);
            sc.jpeg_h = resample ? o.fit_h : h2j_scaled_dim((o.windowed || o.orient) ? o.win_h : f.out_h, sc.scale_log2);
            p.scaled.push_back(sc);
            p.vsrc.push_back(src);
            p.vqscale.push_back(o.pad ? 0 : o.qscale);  // (a padded output's quantiser scale is its canvas's)
            p.vsharpen.push_back(o.sharpen);
            p.qforced = p.qforced || (o.qscale != 0 && !o.pad);
            p.vjpeg.push_back(0);
            p.vpad.push_back(-1);
            p.vcolour.push_back(o.colour);
            p.vcol.push_back(-1);
            p.vshare.push_back(-1);
            const int nv = static_cast<int>(p.scaled.size()) - 1;
            if (!o.colour) return nv;
            // a converted view: the record of an earlier view of the frame with its planes, or a new one; scaled planes
            // an earlier view of the frame has are read, not made again
            for (int u = static_cast<int>(v0); u < nv && p.vcol[nv] < 0; u++)
                if (p.vcol[u] >= 0 && p.vsrc[u] == src && p.vcolour[u] == o.colour && p.scaled[u].scale_log2 == sc.scale_log2 &&
                    p.scaled[u].jpeg_w == sc.jpeg_w && p.scaled[u].jpeg_h == sc.jpeg_h)
                    p.vcol[nv] = p.vcol[u];
            for (int u = static_cast<int>(v0); u < nv && sc.scale_log2 != 0 && p.vshare[nv] < 0; u++)
                if (p.vsrc[u] == src && p.scaled[u].scale_log2 == sc.scale_log2 && p.scaled[u].jpeg_w == sc.jpeg_w && p.scaled[u].jpeg_h == sc.jpeg_h)
                    p.vshare[nv] = p.vshare[u] >= 0 ? p.vshare[u] : u;
            if (p.vcol[nv] < 0) {
                h2j_colour rec{};
                rec.w = sc.jpeg_w;
                rec.h = sc.jpeg_h;
                for (int i = 0; i < 8; i++) rec.k[i] = o.col_k[i];
                rec.matrix = (rec.k[2] | rec.k[3] | rec.k[5] | rec.k[6]) ? 1 : 0;
                p.vcol[nv] = static_cast<int>(p.cols.size());
                p.cols.push_back(rec);
                p.colview.push_back(nv);
            }
            return nv;
        };
        auto canvas_of = [&](const FrameJob::Output& o) {  // the canvas view of a padded output, added if new
            const int pv = view_of(o);
            for (size_t i = 0; i < p.pads.size(); i++) {
                const h2j_pad& rec = p.pads[i];
                if (p.padsrc[i] == pv && rec.bw == o.box_w && rec.bh == o.box_h && rec.px == o.pad_x && rec.py == o.pad_y &&
                    rec.fill[0] == o.fill[0] && rec.fill[1] == o.fill[1] && rec.fill[2] == o.fill[2] &&
                    (p.vqscale[p.padview[i]] == o.qscale || o.format))
                    return p.padview[i];
            }
            h2j_pad rec{};
            rec.w = p.scaled[pv].jpeg_w;
            rec.h = p.scaled[pv].jpeg_h;
            rec.bw = o.box_w;
            rec.bh = o.box_h;
            rec.px = o.pad_x;
            rec.py = o.pad_y;
            for (int c = 0; c < 3; c++) rec.fill[c] = o.fill[c];
            h2j_scaled sc{};
            sc.frame = k;
            sc.jpeg_w = o.box_w;
            sc.jpeg_h = o.box_h;
            p.scaled.push_back(sc);
            p.vsrc.push_back(-1);
            p.vqscale.push_back(o.qscale);
            p.vsharpen.push_back(0);
            p.qforced = p.qforced || o.qscale != 0;
            p.vjpeg.push_back(0);
            p.vpad.push_back(static_cast<int>(p.pads.size()));
            p.vcolour.push_back(0);
            p.vcol.push_back(-1);
            p.vshare.push_back(-1);
            p.pads.push_back(rec);
            p.padsrc.push_back(pv);
            p.padview.push_back(static_cast<int>(p.scaled.size()) - 1);
            return p.padview.back();
        };
        auto rgb_of = [&](int v, int layout) {  // the raw output of view v in this layout, added if new
            for (size_t i = 0; i < p.rgbs.size(); i++)
                if (p.rgbview[i] == v && p.rgbs[i].layout == layout) return static_cast<int>(i);
            h2j_rgb rec{};
            rec.w = p.scaled[v].jpeg_w;
            rec.h = p.scaled[v].jpeg_h;
            rec.layout = layout;
            p.rgbs.push_back(rec);
            p.rgbview.push_back(v);
            return static_cast<int>(p.rgbs.size()) - 1;
        };
        for (int r = 0; r < j.nouts; r++)
            if (j.outs[r].error == 0 && j.outs[r].scale_log2 == 0 && !j.outs[r].windowed && !j.outs[r].orient && !j.outs[r].qscale &&
                !j.outs[r].sharpen && !j.outs[r].colour) {
                view_of(j.outs[r]);
                break;
            }
        // with raw outputs among them the JPEG renditions name their views first, in their order, so that a raw
        // output finds the view of a JPEG rendition with its planes wherever the two stand in the list
        // (likewise with padded outputs: the unpadded JPEG renditions name their views before a padded one looks for
        // its picture part, then the padded JPEG renditions their canvases before a padded raw one looks for one)
        bool raw = false;
        for (int r = 0; r < j.nouts; r++) raw = raw || (j.outs[r].error == 0 && (j.outs[r].format || j.outs[r].pad));
        for (int r = 0; raw && r < j.nouts; r++)
            if (j.outs[r].error == 0 && !j.outs[r].format && !j.outs[r].pad) view_of(j.outs[r]);
        for (int r = 0; raw && r < j.nouts; r++)
            if (j.outs[r].error == 0 && !j.outs[r].format && j.outs[r].pad) canvas_of(j.outs[r]);
        for (int r = 0; r < j.nouts; r++) {
            const FrameJob::Output& o = j.outs[r];
            if (o.error != 0) continue;
            const int v = o.pad ? canvas_of(o) : view_of(o);
            if (!o.format) p.vjpeg[v] = 1;
            p.rends.push_back(ChunkPlan::Rend{j.out_base + r, v, o.format ? rgb_of(v, o.format) : -1});
        }
        d.max_w = std::max(d.max_w, f.width);
        d.max_h = std::max(d.max_h, f.height);
        if (f.codec == H2J_CODEC_HEVC) d.max_ctbs = std::max(d.max_ctbs, f.ctb_w * f.ctb_h);
    }
    p.nv = static_cast<int>(p.scaled.size());
    p.vfirst[p.nf] = p.nv;
    size_t nblk = 0;
    for (const h2j_scaled& sc : p.scaled) {
        d.max_mcu = std::max(d.max_mcu, static_cast<int>(view_blocks(sc) / 6));
        nblk += view_blocks(sc);
    }
    for (int v = 0; v < p.nv; v++)  // the payload estimate: the views that get a JPEG
        if (p.vjpeg[v]) p.px += static_cast<double>(p.scaled[v].jpeg_w) * p.scaled[v].jpeg_h;
    p.tiles = (d.max_mcu * 6 + 255) / 256;
    p.seg_cap = nblk * kSegBytesPerBlock + 16 * static_cast<size_t>(p.nv);
    // the records' places in the staging buffer
    Cursor c;
    p.at.frames = c.take((p.nf + p.wins.size()) * sizeof(h2j_frame));
    p.at.tus = c.take(ntu * sizeof(h2j_tu));
    p.at.coefs = c.take(ncoef * sizeof(h2j_coef));
    p.at.ctbs = c.take(nctb * sizeof(h2j_ctb));
    p.at.slices = c.take(nslice * sizeof(h2j_slice));
    p.at.sl = c.take(nsl + 16);
    p.at.bytes = c.off;  // the maps follow (layout_maps)
}

// arena layout: [zeroed: maps + CTB TU ranges + jstat][pic][pic2][spic][opic][vpic][upic][bpic][rgb][jcoef][res][aux]
void layout_arena(ChunkPlan& p) {
    Cursor a;
    for (h2j_frame& f : p.frames) {
        f.maps = a.take(static_cast<size_t>(f.mw) * f.mh * 2);
        f.ctbrng = a.take(static_cast<size_t>(f.ctb_w) * f.ctb_h * 16);  // [first, first chroma, end, -]
    }
    p.jstat_base = a.off;
    p.jstat_stride = align_up(sizeof(h2j_jstat), 256);
    for (int v = 0; v < p.nv; v++) {  // one per view; a frame's own is its first view's
        h2j_scaled& sc = p.scaled[v];
        sc.jstat = a.take(p.jstat_stride);
        if (v == p.vfirst[sc.frame]) p.frames[sc.frame].jstat = sc.jstat;
    }
    p.njstat = p.nv;
    for (int k = 0; k < p.nf; k++) {  // ... unless that view is an unscaled window (ChunkPlan::fstat)
        const int v = p.vfirst[k];
        p.fstat[k] = v;
        if (p.vsrc[v] == k || p.scaled[v].scale_log2 != 0) continue;
        p.fstat[k] = p.njstat++;
        p.frames[k].jstat = a.take(p.jstat_stride);
    }
    p.zero_bytes = a.off;
    for (int pass = 0; pass < 2; pass++)
        for (h2j_frame& f : p.frames) {
            const size_t pel = f.bit_depth > 8 ? 2 : 1;
            const size_t ysz = static_cast<size_t>(f.width) * f.height, csz = ysz / 4;
            f.pic_stride[0] = f.width;
            f.pic_stride[1] = f.pic_stride[2] = f.width / 2;
            f.pic_off[0] = 0;
            f.pic_off[1] = static_cast<int32_t>(ysz);
            f.pic_off[2] = static_cast<int32_t>(ysz + csz);
            if (pass == 1 && (f.codec != H2J_CODEC_HEVC || !f.sao_enabled)) {
                f.pic2 = f.pic;  // no SAO: the deblocked picture is the decoded picture (K3 skips it)
                continue;
            }
            (pass == 0 ? f.pic : f.pic2) = a.take((ysz + 2 * csz) * pel);
        }
    for (size_t v = 0; v < p.scaled.size(); v++) {  // the 8-bit scaled planes K3s / K3r / K3p write and K4 reads (scaled views only)
        h2j_scaled& sc = p.scaled[v];
        if (sc.scale_log2 == 0) continue;
        if (p.vshare[v] >= 0) {  // (a converted view that reads an earlier view's)
            const h2j_scaled& su = p.scaled[p.vshare[v]];
            sc.spic = su.spic;
            for (int c = 0; c < 3; c++) {
                sc.spic_stride[c] = su.spic_stride[c];
                sc.spic_off[c] = su.spic_off[c];
            }
            continue;
        }
        size_t po = 0;
        for (int c = 0; c < 3; c++) {
            const int pw = c ? sc.jpeg_w / 2 : sc.jpeg_w, ph = c ? sc.jpeg_h / 2 : sc.jpeg_h;
            sc.spic_stride[c] = h2j_spic_stride(pw);
            sc.spic_off[c] = static_cast<int32_t>(po);
            po += static_cast<size_t>(sc.spic_stride[c]) * ph;
        }
        sc.spic = a.take(po);
    }
    for (h2j_orient& rec : p.orients) {  // the oriented planes K3o writes, in the frame's sample type
        const h2j_frame& f = p.frames[rec.frame];
        const int pel = f.bit_depth > 8 ? 2 : 1;
        const int ow = rec.orient >= 5 ? f.out_h : f.out_w, oh = rec.orient >= 5 ? f.out_w : f.out_h;
        size_t po = 0;  // elements; every plane starts on a 64-byte boundary
        for (int c = 0; c < 3; c++) {
            rec.stride[c] = h2j_opic_stride(c ? ow / 2 : ow, pel);
            rec.off[c] = static_cast<int32_t>(po);
            po += static_cast<size_t>(rec.stride[c]) * (c ? oh / 2 : oh);
        }
        rec.opic = a.take(po * pel);
    }
    p.colour_bytes = 0;
    for (size_t i = 0; i < p.cols.size(); i++) {  // the 8-bit converted planes K3v writes (converted views only)
        h2j_colour& rec = p.cols[i];
        rec.jstat = p.scaled[p.colview[i]].jstat;
        size_t po = 0;
        for (int c = 0; c < 3; c++) {
            rec.dst_stride[c] = h2j_spic_stride(c ? rec.w / 2 : rec.w);
            rec.dst_off[c] = static_cast<int32_t>(po);
            po += static_cast<size_t>(rec.dst_stride[c]) * (c ? rec.h / 2 : rec.h);
        }
        rec.dst = a.take(po);
        p.colour_bytes += po;
    }
    for (int v = 0; v < p.nv; v++) {  // the 8-bit sharpened planes K3u writes and K4 reads (sharpened views only)
        p.vfin[v] = -1;
        if (!p.vsharpen[v]) continue;
        const h2j_scaled& sc = p.scaled[v];
        h2j_finish rec{};
        rec.w = sc.jpeg_w;
        rec.h = sc.jpeg_h;
        rec.sharpen = p.vsharpen[v];
        rec.jstat = sc.jstat;
        size_t po = 0;
        for (int c = 0; c < 3; c++) {
            rec.dst_stride[c] = h2j_spic_stride(c ? rec.w / 2 : rec.w);
            rec.dst_off[c] = static_cast<int32_t>(po);
            po += static_cast<size_t>(rec.dst_stride[c]) * (c ? rec.h / 2 : rec.h);
        }
        rec.dst = a.take(po);
        p.vfin[v] = static_cast<int>(p.fins.size());
        p.fins.push_back(rec);
    }
    p.pad_bytes = 0;
    for (h2j_pad& rec : p.pads) {  // the 8-bit canvas planes K3b writes and K4 / K3c read (padded outputs only)
        size_t po = 0;
        for (int c = 0; c < 3; c++) {
            rec.dst_stride[c] = h2j_spic_stride(c ? rec.bw / 2 : rec.bw);
            rec.dst_off[c] = static_cast<int32_t>(po);
            po += static_cast<size_t>(rec.dst_stride[c]) * (c ? rec.bh / 2 : rec.bh);
        }
        rec.dst = a.take(po);
        p.pad_bytes += po;
    }
    p.rgb_base = a.off;  // the RGB pixels K3c writes (raw outputs only): one region, each output 256-byte aligned
    for (h2j_rgb& rec : p.rgbs) rec.dst_off = a.take(3 * static_cast<size_t>(rec.w) * rec.h);
    p.rgb_bytes = a.off - p.rgb_base;
    for (int v = 0; v < p.nv; v++) {  // per view: dense int16 plane (inspection) or the JPEG symbol tiles
        const h2j_scaled& sc = p.scaled[v];
        const size_t blocks = view_blocks(sc);
        p.vjcoef[v] = a.take(std::max(blocks * 64 * 2, (blocks + 255) / 256 * static_cast<size_t>(H2J_JTILE_BYTES)));
        if (v == p.vfirst[sc.frame]) p.frames[sc.frame].jcoef = p.vjcoef[v];
    }
    for (h2j_frame& f : p.frames) {
        const size_t ysz = static_cast<size_t>(f.width) * f.height;
        // HEVC residual planes are tiled by K1 quadrant (include/h2j_gpu.h h2j_res_elems: whole
        // tiles, a little more than the picture); H.264 keeps the picture's raster layout
        const size_t res_elems = f.codec == H2J_CODEC_HEVC
                                     ? static_cast<size_t>(h2j_res_elems(f.width, f.height, f.log2ctb))
                                     : ysz + ysz / 2;
        f.res = a.take(res_elems * 2);
        f.aux = a.take(static_cast<size_t>(f.ntu) * 8);
        if (f.k1bands > 1) {  // per band boundary: K1 1 luma + 2 chroma rows, K2 4 luma + 2x2 chroma rows (uint16)
            // K1's 8-row bands and K2's 16-row bands use it one after the other
            const size_t k2b = static_cast<size_t>(f.k1bands - 1) * 6 * f.width * 2;
            const size_t k1b = static_cast<size_t>((f.ctb_h + 7) / 8 - 1) * 2 * f.width * 2;
            f.xline = a.take(std::max(k1b, k2b));
        }
    }
    p.arena_bytes = a.off;
}

// the banded H.264 pictures' bands of `rows` macroblock rows, band-major: (frame << 8) | band
void band_major(const std::vector<h2j_frame>& frames, int rows, std::vector<uint32_t>& map) {
    int maxb = 0;
    for (const h2j_frame& f : frames)
        if (banded(f)) maxb = std::max(maxb, (f.ctb_h + rows - 1) / rows);
    for (int bnd = 0; bnd < maxb; bnd++)
        for (size_t k = 0; k < frames.size(); k++)
            if (banded(frames[k]) && bnd < (frames[k].ctb_h + rows - 1) / rows)
                map.push_back((static_cast<uint32_t>(k) << 8) | static_cast<uint32_t>(bnd));
}

void build_k1_maps(ChunkPlan& p) {
    // H.264 K1 workgroup map: banded pictures first (their long chains start early), bands in order,
    // then the others by transform-block count, most first (the dispatcher hands workgroups out in
    // map order: the heaviest pictures start in the first round, not in the launch's tail)
    // Banded pictures band-major (every picture's band 0, then every band 1, ...): a band waits on
    // the band above, and picture-major order had each picture's lower bands holding workgroup
    // slots while they waited (a batch of 4K H.264 pictures ran at a fraction of the GPU).  A band
    // still follows the band above it in the map, so it never waits on one not yet dispatched.
    band_major(p.frames, 16, p.k1map);  // k1bands bands of 16 rows
    // the same for h2j_k1_recon_h264's 8-wave workgroups: bands of 8 rows (16-row bands took two
    // row rounds each, so a band below started a whole row time after the band above)
    band_major(p.frames, 8, p.k1map8);
    Keyed e;
    for (int k = 0; k < p.nf; k++) {
        const h2j_frame& f = p.frames[k];
        if (f.codec == H2J_CODEC_H264 && !banded(f)) e.emplace_back(-static_cast<long long>(f.ntu), static_cast<uint32_t>(k) << 8);
    }
    const size_t nbanded = p.k1map.size();
    append_by_key(e, p.k1map);
    p.k1map8.insert(p.k1map8.end(), p.k1map.begin() + static_cast<long>(nbanded), p.k1map.end());
    // mixed-batch K1 map (h2j_k1_recon_any): every HEVC picture and H.264 band, tallest first so
    // the longest chains start first; bands of one picture stay in order
    e.clear();
    for (int k = 0; k < p.nf; k++) {
        const h2j_frame& f = p.frames[k];
        if (f.codec != H2J_CODEC_HEVC) continue;
        const int rows = f.ctb_h << (f.log2ctb - 4);  // in 16-sample rows
        if (rows > kK1BandRows) {  // taller than 1088: a 16-wave workgroup per component group
            e.emplace_back(-2000 - rows, (3u << 30) | (static_cast<uint32_t>(k) << 8) | 0u);
            e.emplace_back(-2000 - rows, (3u << 30) | (static_cast<uint32_t>(k) << 8) | 1u);
        } else {
            e.emplace_back(-rows, (1u << 31) | (static_cast<uint32_t>(k) << 8));
        }
    }
    for (uint32_t m : p.k1map) {
        const h2j_frame& f = p.frames[m >> 8];
        e.emplace_back(-std::min(f.ctb_h, 16) - (f.k1bands > 1 ? 1000 : 0), m);
    }
    append_by_key(e, p.k1all);
    for (uint32_t m : p.k1all)
        if (m & 0x80000000u) p.k1hevc.push_back(m);
}

// K3 SAO map: the HEVC pictures with SAO, most CTBs first, cut into CTB-count classes (a picture
// joins the current class while it has more than half the class's CTBs; the last class takes
// the rest), one launch each, so no class pays for the largest picture's grid width
void build_sao_classes(ChunkPlan& p) {
    h2j_gpu_batch& d = p.desc;
    Keyed e;
    for (int k = 0; k < p.nf; k++) {
        const h2j_frame& f = p.frames[k];
        if (f.codec == H2J_CODEC_HEVC && f.pic2 != f.pic) e.emplace_back(-static_cast<long long>(f.ctb_w * f.ctb_h), static_cast<uint32_t>(k));
    }
    append_by_key(e, p.saomap);
    for (size_t i = 0; i < e.size(); i++) {  // e is now in map order: entry i is saomap[i], its key -CTBs
        const int ctbs = static_cast<int>(-e[i].first);
        const bool same = d.sao_groups > 0 && (d.sao_groups == H2J_SAO_GROUPS || 2 * ctbs > d.sao_ctbs[d.sao_groups - 1]);
        if (!same) {
            d.sao_first[d.sao_groups] = static_cast<int>(i);
            d.sao_ctbs[d.sao_groups] = ctbs;
            d.sao_groups++;
        }
        d.sao_count[d.sao_groups - 1]++;
    }
}

// K3s / K3r map: the scaled pictures by class (K3s: sample type x scale, K3r: sample type), one
// launch per class present, its grid as wide as the class's largest picture needs
// K3p map: a frame with two or more K3s levels among its views gets one h2j_pyramid instead of a K3s
// entry per level, by class (sample type, coarsest level)
void build_scale_classes(ChunkPlan& p) {
    h2j_gpu_batch& d = p.desc;
    // per source (a frame, or nf + a window: the index the kernels find it under): mask of its K3s levels
    const int ns = p.nf + static_cast<int>(p.wins.size());
    std::vector<int> levels(static_cast<size_t>(ns), 0);
    int npyr = 0;
    for (int v = 0; v < p.nv && p.nv > p.nf; v++)
        if (k3s_level(p.scaled[v])) levels[p.vsrc[v]] |= 1 << p.scaled[v].scale_log2;
    for (int k = 0; k < ns; k++) {
        if (levels[k] & (levels[k] - 1)) npyr++;
        else levels[k] = 0;  // one level: K3s
    }
    // a pyramid writes one view a level: the source's first at that level.  Later views of the same source and
    // level -- they differ from it in qscale or sharpen only -- have planes of their own, written by K3s
    auto in_pyramid = [&](int v) {
        const h2j_scaled& sc = p.scaled[v];
        if (!k3s_level(sc) || !((levels[p.vsrc[v]] >> sc.scale_log2) & 1)) return false;
        for (int u = p.vfirst[sc.frame]; u < v; u++)
            if (p.vsrc[u] == p.vsrc[v] && p.scaled[u].scale_log2 == sc.scale_log2) return false;
        return true;
    };
    for (int cls = 0; cls < H2J_PYR_CLASSES && npyr; cls++) {
        d.pyr_first[cls] = static_cast<int>(p.pyrmap.size());
        for (int k = 0; k < ns; k++) {
            if (!levels[k]) continue;
            const int fr = k < p.nf ? k : p.wins[k - p.nf].frame;
            const int kc = (levels[k] & 8) ? 3 : 2;
            if (2 * (p.frames[fr].bit_depth > 8 ? 1 : 0) + kc - 2 != cls) continue;
            h2j_pyramid py{};
            py.frame = k;
            py.mask = levels[k];
            for (int v = p.vfirst[fr]; v < p.vfirst[fr + 1]; v++)
                if (p.vsrc[v] == k && in_pyramid(v)) {
                    py.lvl[p.scaled[v].scale_log2 - 1] = p.scaled[v];
                    py.lvl[p.scaled[v].scale_log2 - 1].frame = k;
                }
            p.pyrmap.push_back(py);
            d.pyr_count[cls]++;
            d.pyr_tiles[cls] = std::max(d.pyr_tiles[cls], h2j_k3s_tiles(py.lvl[kc - 1].jpeg_w, py.lvl[kc - 1].jpeg_h));
        }
    }
    for (int cls = 0; cls < H2J_SCALE_CLASSES && p.views; cls++) {
        d.scale_first[cls] = static_cast<int>(p.scalemap.size());
        for (int v = 0; v < p.nv; v++) {
            const h2j_scaled& sc = p.scaled[v];
            if (sc.scale_log2 == 0 || in_pyramid(v) || p.vshare[v] >= 0) continue;  // unscaled, K3p's, or another view's planes
            const int hbd = p.frames[sc.frame].bit_depth > 8 ? 1 : 0;
            const bool resample = sc.scale_log2 == H2J_SCALE_RESAMPLE;
            if ((resample ? H2J_K3R_CLASS0 + hbd : 3 * hbd + sc.scale_log2 - 1) != cls) continue;
            p.scalemap.push_back(sc);
            p.scalemap.back().frame = p.vsrc[v];  // the kernel's source: the frame, or the window's copy of it
            d.scale_count[cls]++;
            d.scale_tiles[cls] = std::max(d.scale_tiles[cls], resample ? h2j_k3r_tiles(sc.jpeg_w, sc.jpeg_h) : h2j_k3s_tiles(sc.jpeg_w, sc.jpeg_h));
        }
    }
}

// the source half of a K3u, K3b or K3c record (the fields have the same names in all three): the planes the stage reads,
// as the view `src` shows them; wide: the 8-bit planes a scale or finishing kernel wrote (aligned dword loads)
template <typename Rec>
void fill_source(Rec& rec, const h2j_frame& src, bool wide) {
    rec.bit_depth = src.bit_depth;
    rec.bit_depth_c = src.bit_depth_c;
    rec.crop_x = src.crop_x;
    rec.crop_y = src.crop_y;
    rec.wide = wide ? 1 : 0;
    rec.src = src.pic2;
    for (int c = 0; c < 3; c++) {
        rec.src_stride[c] = src.pic_stride[c];
        rec.src_off[c] = src.pic_off[c];
    }
}
// the class of a K3u, K3b or K3c record: 0: the 8-bit planes K3s / K3r / K3p (/ K3u) wrote; 1: another 8-bit source; 2: a
// 16-bit source
template <typename Rec>
int source_class(const Rec& rec) { return rec.wide ? 0 : rec.bit_depth > 8 ? 2 : 1; }

// The late stages' maps (ChunkPlan::StageMap), each grouped by class, one launch per class present, its grid as wide
// as the class's largest picture needs
void build_late_stage_maps(ChunkPlan& p) {
    // K3o: the oriented sources, by sample type x transposing
    p.orientmap.group(p.orients,
                      [&](const h2j_orient& rec) { return 2 * (p.frames[rec.frame].bit_depth > 8 ? 1 : 0) + (rec.orient >= 5 ? 1 : 0); },
                      [&](const h2j_orient& rec) {
                          const h2j_frame& f = p.frames[rec.frame];
                          const bool tr = rec.orient >= 5;
                          return h2j_k3o_tiles(tr ? f.out_h : f.out_w, tr ? f.out_w : f.out_h, f.bit_depth > 8 ? 2 : 1, tr);
                      });
    // K3v: the converted outputs with their sources (what each view is without colour and sharpening)
    for (size_t i = 0; i < p.cols.size(); i++) {
        const int v = p.colview[i];
        fill_source(p.cols[i], p.scaled_view(v), p.scaled[v].scale_log2 != 0);
    }
    p.colmap.group(p.cols, [](const h2j_colour& rec) { return 2 * source_class(rec) + (rec.matrix ? 1 : 0); },
                   [](const h2j_colour& rec) { return rec.matrix ? h2j_k3v_matrix_tiles(rec.w, rec.h) : h2j_k3v_range_tiles(rec.w, rec.h); });
    // K3u: the sharpened outputs with their sources (what each view is without its sharpening)
    for (int v = 0; v < p.nv; v++)
        if (p.vfin[v] >= 0) fill_source(p.fins[p.vfin[v]], p.base_view(v), p.scaled[v].scale_log2 != 0 || p.vcol[v] >= 0);
    p.finmap.group(p.fins, source_class<h2j_finish>, [](const h2j_finish& rec) { return h2j_k3u_tiles(rec.w, rec.h); });
    // K3b: the canvases with their sources (what view() shows K4 of the picture part)
    for (size_t i = 0; i < p.pads.size(); i++) {
        const int v = p.padsrc[i];
        fill_source(p.pads[i], p.view(v), p.scaled[v].scale_log2 != 0 || p.vfin[v] >= 0 || p.vcol[v] >= 0);
    }
    p.padmap.group(p.pads, source_class<h2j_pad>, [](const h2j_pad& rec) { return h2j_k3b_tiles(rec.bw, rec.bh); });
    // K3c: the raw outputs with their sources (what view() shows K4; a canvas is wide)
    for (size_t i = 0; i < p.rgbs.size(); i++) {
        const int v = p.rgbview[i];
        fill_source(p.rgbs[i], p.view(v), p.scaled[v].scale_log2 != 0 || p.vfin[v] >= 0 || p.vpad[v] >= 0 || p.vcol[v] >= 0);
    }
    p.rgbmap.group(p.rgbs, source_class<h2j_rgb>, [](const h2j_rgb& rec) { return h2j_k3c_tiles(rec.w, rec.h); });
}

// the maps' places in the staging buffer, behind the records; with scaled pictures or several
// renditions of a frame the JPEG source views of all frames and the K3s / K3r / K3p maps follow
void layout_maps(ChunkPlan& p) {
    Cursor c;
    c.off = p.at.bytes;
    p.at.k1map = c.take(p.k1map.size() * 4 + 16);
    p.at.k1all = c.take(p.k1all.size() * 4 + 16);
    p.at.sao = c.take(p.saomap.size() * 4 + 16);
    p.at.k1map8 = c.take(p.k1map8.size() * 4 + 16);
    p.at.k1hevc = c.take(p.k1hevc.size() * 4 + 16);
    p.at.jframes = p.at.scale = c.off;
    if (p.views) {
        p.at.jframes = c.take(p.nv * sizeof(h2j_frame));
        p.at.scale = c.take(p.scalemap.size() * sizeof(h2j_scaled) + 16);
    }
    p.at.pyr = c.off;
    if (!p.pyrmap.empty()) c.take(p.pyrmap.size() * sizeof(h2j_pyramid) + 16);
    // the late stages' maps, each only in chunks that have the stage: every offset above is what it was
    p.orientmap.at = c.take(p.orientmap.staging_bytes());
    p.finmap.at = c.take(p.finmap.staging_bytes());
    p.at.qforce = c.off;  // only in chunks with a forced quantiser scale: one int32 a view
    if (p.qforced) c.take(static_cast<size_t>(p.nv) * 4 + 16);
    p.rgbmap.at = c.take(p.rgbmap.staging_bytes());
    p.at.jcompact = c.off;  // only in chunks with views that get no JPEG: the views K4 / K5 run on
    if (p.compact()) c.take(static_cast<size_t>(p.njpeg) * sizeof(h2j_frame));
    p.padmap.at = c.take(p.padmap.staging_bytes());  // behind everything else
    p.colmap.at = c.take(p.colmap.staging_bytes());  // ... and the youngest behind that
    p.at.bytes = c.off;
}

// the descriptor's counts and masks (the maxima and the classes are set where they are found)
void fill_descriptor(ChunkPlan& p) {
    h2j_gpu_batch& d = p.desc;
    d.nframes = p.nf;
    for (const h2j_frame& f : p.frames) {
        if (f.codec == H2J_CODEC_HEVC) {
            d.has_hevc = 1;
            d.hevc_pels |= (f.bit_depth > 8 || f.bit_depth_c > 8) ? 2 : 1;
        }
        if (f.codec != H2J_CODEC_H264) continue;
        d.has_h264 = 1;
        if (f.mbaff) d.has_mbaff = 1;
        else d.h264_pels |= f.bit_depth == 8 ? 1 : 2;
    }
    d.k1wgs = static_cast<int32_t>(p.k1map.size());
    d.k1all_n = static_cast<int32_t>(p.k1all.size());
    d.k1wgs8 = static_cast<int32_t>(p.k1map8.size());
    d.k1hevc_n = static_cast<int32_t>(p.k1hevc.size());
    // pictures whose MB variances K4a sums (K3 sums the others'; no K4a launch when none is left)
    // (a scaled picture: always K4a, on the scaled picture; K3s / K3r clears what K3 may have summed)
    // (a window: always K4a, on the window; a sharpened view: always K4a, on the sharpened planes)
    for (int v = 0; v < p.nv; v++)
        if (p.vjpeg[v])  // (K4 runs on the views that get a JPEG)
            d.k4a_frames += (h2j_sao_folds_variance(p.frames[p.scaled[v].frame]) && p.scaled[v].scale_log2 == 0 && p.vsrc[v] < p.nf && !p.vsharpen[v] &&
                             p.vpad[v] < 0 && p.vcol[v] < 0) ? 0 : 1;  // (a canvas, a converted view: always K4a, on those planes)
}

}  // namespace

// An unscaled frame is its own view; a scaled frame's view is the 8-bit picture K3s, K3r or K3p writes
// at its h2j_scaled record's spic (include/h2j_gpu.h h2j_gpu_batch.jframes).  Every view has its own
// jcoef / tile region and jstat (the first view keeps the frame's own).
// A sharpened view is the 8-bit picture K3u writes at its h2j_finish record's dst, from what the view is without
// the sharpening (base_view)
// A canvas view is the 8-bit picture K3b writes at its h2j_pad record's dst
h2j_frame ChunkPlan::view(int v) const {
    // f with the w x h 8-bit planes a late stage wrote at dst for its picture (pic == pic2: K4a sums their MB variances)
    auto shows = [](h2j_frame f, uint64_t dst, int w, int h, const int32_t* stride, const int32_t* off) {
        f.pic = f.pic2 = dst;
        f.crop_x = f.crop_y = 0;
        f.out_w = w;
        f.out_h = h;
        f.bit_depth = f.bit_depth_c = 8;
        for (int c = 0; c < 3; c++) {
            f.pic_stride[c] = stride[c];
            f.pic_off[c] = off[c];
        }
        return f;
    };
    const h2j_frame f = base_view(v);
    if (vpad[v] >= 0) {
        const h2j_pad& rec = pads[vpad[v]];
        return shows(f, rec.dst, rec.bw, rec.bh, rec.dst_stride, rec.dst_off);
    }
    if (vfin[v] < 0) return f;
    const h2j_finish& rec = fins[vfin[v]];
    return shows(f, rec.dst, rec.w, rec.h, rec.dst_stride, rec.dst_off);
}

// A converted view is the 8-bit picture K3v writes at its h2j_colour record's dst, from what the view is without the
// conversion (scaled_view)
h2j_frame ChunkPlan::base_view(int v) const {
    h2j_frame f = scaled_view(v);
    if (vcol[v] < 0) return f;
    const h2j_colour& rec = cols[vcol[v]];
    f.pic = f.pic2 = rec.dst;  // pic == pic2: K4a sums the converted picture's MB variances
    f.crop_x = f.crop_y = 0;
    f.out_w = rec.w;
    f.out_h = rec.h;
    f.bit_depth = f.bit_depth_c = 8;
    for (int c = 0; c < 3; c++) {
        f.pic_stride[c] = rec.dst_stride[c];
        f.pic_off[c] = rec.dst_off[c];
    }
    return f;
}

h2j_frame ChunkPlan::scaled_view(int v) const {
    const h2j_scaled& sc = scaled[v];
    h2j_frame f = frames[sc.frame];
    f.jcoef = vjcoef[v];
    f.jstat = sc.jstat;
    if (sc.scale_log2 == 0 && vsrc[v] >= nf) {  // an unscaled window: the frame in place, its crop moved
        const h2j_frame w = wframe(vsrc[v] - nf);
        f.crop_x = w.crop_x;
        f.crop_y = w.crop_y;
        f.out_w = w.out_w;
        f.out_h = w.out_h;
        f.pic = f.pic2;  // pic == pic2: K4a sums the window's MB variances (K3 SAO summed the whole picture's)
        if (wins[vsrc[v] - nf].osrc >= 0) {  // ... of an oriented source: the oriented planes in place
            f.pic = f.pic2 = w.pic2;
            for (int c = 0; c < 3; c++) {
                f.pic_stride[c] = w.pic_stride[c];
                f.pic_off[c] = w.pic_off[c];
            }
        }
    }
    if (sc.scale_log2 == 0) return f;
    f.pic = f.pic2 = sc.spic;  // pic == pic2: K4a sums its MB variances (h2j_sao_folds_variance)
    f.crop_x = f.crop_y = 0;
    f.out_w = sc.jpeg_w;
    f.out_h = sc.jpeg_h;
    f.bit_depth = f.bit_depth_c = 8;
    for (int c = 0; c < 3; c++) {
        f.pic_stride[c] = sc.spic_stride[c];
        f.pic_off[c] = sc.spic_off[c];
    }
    return f;
}

h2j_frame ChunkPlan::wframe(int j) const {
    const Window& w = wins[j];
    h2j_frame f = frames[w.frame];
    if (w.osrc >= 0) {  // the window lies in the oriented planes K3o wrote: pic == pic2, no conformance crop
        const h2j_orient& rec = orients[w.osrc];
        f.pic = f.pic2 = rec.opic;
        f.crop_x = f.crop_y = 0;
        for (int c = 0; c < 3; c++) {
            f.pic_stride[c] = rec.stride[c];
            f.pic_off[c] = rec.off[c];
        }
    }
    f.crop_x += w.x;
    f.crop_y += w.y;
    f.out_w = w.w;
    f.out_h = w.h;
    return f;
}

inline void clear_all() {}
template <typename V, typename... Vs>
void clear_all(V& v, Vs&... vs) {
    v.clear();
    clear_all(vs...);
}

void ChunkPlan::reset(int nframes) {
    nf = nframes;
    frames.resize(static_cast<size_t>(nf));
    vfirst.assign(static_cast<size_t>(nf) + 1, 0);
    fstat.assign(static_cast<size_t>(nf), 0);
    clear_all(k1map, k1map8, k1all, k1hevc, saomap, scaled, scalemap, pyrmap, vsrc, wins, rends, jviews);
    clear_all(orients, orientmap, vqscale, vsharpen, fins, finmap, rgbs, rgbview, rgbmap, vjpeg, vpad, pads, padview, padsrc, padmap);
    clear_all(vcolour, vcol, vshare, cols, colview, colmap);
    qforced = false;
    px = 0;
    std::memset(&desc, 0, sizeof(desc));
}

void plan_chunk(const std::vector<FrameJob>& jobs, const std::vector<int>& live, ChunkPlan& p) {
    p.reset(static_cast<int>(live.size()));
    number_frames_and_views(jobs, live, p);
    // scaled pictures present, or several renditions of a frame: a views array is uploaded
    p.views = p.nv > p.nf || !p.wins.empty() || std::any_of(p.scaled.begin(), p.scaled.end(), [](const h2j_scaled& sc) { return sc.scale_log2 != 0; }) ||
              std::any_of(p.vsharpen.begin(), p.vsharpen.end(), [](int a) { return a != 0; }) ||  // ... or a sharpened view
              !p.cols.empty();  // ... or a converted one
    p.njpeg = static_cast<int>(std::count(p.vjpeg.begin(), p.vjpeg.end(), 1));
    for (int v = 0; v < p.nv && p.compact(); v++)
        if (p.vjpeg[v]) p.jviews.push_back(v);
    p.vjcoef.resize(static_cast<size_t>(p.nv));
    p.vfin.assign(static_cast<size_t>(p.nv), -1);
    layout_arena(p);
    build_k1_maps(p);
    build_sao_classes(p);
    build_scale_classes(p);
    build_late_stage_maps(p);
    layout_maps(p);
    fill_descriptor(p);
}

}  // namespace h2j
