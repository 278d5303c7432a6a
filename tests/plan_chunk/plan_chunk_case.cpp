// plan_chunk on the host (tests/test_crop_api.py): a frame whose renditions name two windows and the whole
// picture, planned without an engine or a GPU; prints what the plan holds, one `key value...` line each.
#include <cstdio>
#include <vector>

#include "chunk_plan.h"

using namespace h2j;

static FrameJob::Output out(int k, int x, int y, int w, int h, bool windowed) {
    FrameJob::Output o;
    o.scale_log2 = k;
    o.win_x = x;
    o.win_y = y;
    o.win_w = w;
    o.win_h = h;
    o.windowed = windowed;
    return o;
}

int main() {
    std::vector<FrameJob> jobs(2);
    for (FrameJob& j : jobs) {  // a 416 x 240 8-bit HEVC picture with SAO, CTB 16, conformance crop (0, 0)
        h2j_frame& f = j.hdr;
        f.codec = H2J_CODEC_HEVC;
        f.width = f.out_w = 416;
        f.height = f.out_h = 240;
        f.bit_depth = f.bit_depth_c = 8;
        f.log2ctb = 4;
        f.ctb_w = 26;
        f.ctb_h = 15;
        f.sao_enabled = 1;
        f.mw = 104;
        f.mh = 60;
        j.tus.resize(4);
        j.ctbs.resize(26 * 15);
        j.slices.resize(1);
    }
    // frame 0: window A at scales 1, 2, 3; window B at scale 1; the whole picture at scale 0 (asked for last)
    FrameJob& a = jobs[0];
    a.nouts = 5;
    a.outs[0] = out(1, 36, 10, 300, 200, true);
    a.outs[1] = out(2, 36, 10, 300, 200, true);
    a.outs[2] = out(3, 36, 10, 300, 200, true);
    a.outs[3] = out(1, 2, 6, 44, 36, true);
    a.outs[4] = out(0, 0, 0, 416, 240, false);
    a.out_base = 0;
    // frame 1: an unscaled 16-aligned window as the only rendition (the variance-fold trap)
    FrameJob& b = jobs[1];
    b.nouts = 1;
    b.outs[0] = out(0, 16, 16, 64, 48, true);
    b.out_base = 5;
    ChunkPlan p;
    plan_chunk(jobs, std::vector<int>{0, 1}, p);
    std::printf("nf %d nv %d njstat %d wins %zu views %d\n", p.nf, p.nv, p.njstat, p.wins.size(), p.views ? 1 : 0);
    for (int v = 0; v < p.nv; v++)
        std::printf("view %d frame %d src %d scale %d size %d %d\n", v, p.scaled[v].frame, p.vsrc[v], p.scaled[v].scale_log2,
                    p.scaled[v].jpeg_w, p.scaled[v].jpeg_h);
    for (const ChunkPlan::Rend& r : p.rends) std::printf("rend %d view %d\n", r.out, r.view);
    for (const h2j_pyramid& py : p.pyrmap) std::printf("pyramid frame %d mask %d sizes %d %d %d\n", py.frame, py.mask, py.lvl[0].jpeg_w, py.lvl[1].jpeg_w, py.lvl[2].jpeg_w);
    for (const h2j_scaled& sc : p.scalemap) std::printf("k3s frame %d scale %d size %d %d\n", sc.frame, sc.scale_log2, sc.jpeg_w, sc.jpeg_h);
    for (size_t j = 0; j < p.wins.size(); j++) {
        const h2j_frame w = p.wframe(static_cast<int>(j));
        std::printf("wframe %zu crop %d %d out %d %d pic2 %d\n", j, w.crop_x, w.crop_y, w.out_w, w.out_h, w.pic2 == p.frames[p.wins[j].frame].pic2);
    }
    const h2j_frame v5 = p.view(5), f1 = p.frames[1];
    std::printf("window_view crop %d %d out %d %d pic_is_pic2 %d own_jstat %d frame_folds %d view_folds %d\n", v5.crop_x, v5.crop_y,
                v5.out_w, v5.out_h, v5.pic == v5.pic2, v5.jstat != f1.jstat, h2j_sao_folds_variance(f1) ? 1 : 0,
                h2j_sao_folds_variance(v5) ? 1 : 0);
    std::printf("fstat %d %d k4a_frames %d staging_frames %zu\n", p.fstat[0], p.fstat[1], p.desc.k4a_frames,
                (p.at.tus - p.at.frames) / sizeof(h2j_frame));
    return 0;
}
