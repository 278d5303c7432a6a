// HEIF / HEIC demuxer (heif.h).  The box nesting read is file -> meta -> { hdlr, pitm, iinf -> infe, iloc, idat,
// iref -> references, iprp -> { ipco -> properties, ipma } }: every level is a loop in a function of its own, so
// nothing here recurses.  All positions are 64-bit offsets into the caller's buffer, compared against the
// enclosing box before a byte is read.
#include "heif.h"

namespace h2j {
namespace {

constexpr uint32_t cc4(char a, char b, char c, char d) {
    return (static_cast<uint32_t>(static_cast<uint8_t>(a)) << 24) | (static_cast<uint32_t>(static_cast<uint8_t>(b)) << 16) |
           (static_cast<uint32_t>(static_cast<uint8_t>(c)) << 8) | static_cast<uint32_t>(static_cast<uint8_t>(d));
}

// big-endian reader over d[pos, end): a read past the end sets bad and returns 0 from then on
struct Rd {
    const uint8_t* d;
    uint64_t pos, end;
    bool bad;
    Rd(const uint8_t* d_, uint64_t pos_, uint64_t end_) : d(d_), pos(pos_), end(end_), bad(false) {}
    uint64_t left() const { return end - pos; }
    uint64_t be(int bytes) {
        if (bad || left() < static_cast<uint64_t>(bytes)) {
            bad = true;
            return 0;
        }
        uint64_t v = 0;
        for (int i = 0; i < bytes; i++) v = (v << 8) | d[pos + i];
        pos += bytes;
        return v;
    }
    void skip(uint64_t k) {
        if (bad || left() < k) bad = true;
        else pos += k;
    }
};

struct Box {
    uint32_t type;
    uint64_t body, end;  // payload d[body, end)
};

// the next box of r's range; false at its end, or with r.bad for a header that does not fit the range
bool next_box(Rd& r, Box& b) {
    if (r.bad || r.left() == 0) return false;
    const uint64_t start = r.pos;
    uint64_t size = r.be(4), hdr = 8;
    b.type = static_cast<uint32_t>(r.be(4));
    if (size == 1) {
        size = r.be(8);
        hdr = 16;
    } else if (size == 0) {
        size = r.end - start;
    }
    if (r.bad || size < hdr || size > r.end - start) {
        r.bad = true;
        return false;
    }
    b.body = start + hdr;
    b.end = start + size;
    r.pos = b.end;
    return true;
}

struct Extent {
    uint64_t off, len;
};
struct Item {
    uint32_t id, type;
    bool located;
    uint32_t method, dref;
    uint64_t base;
    std::vector<Extent> ext;
};
struct Prop {
    uint32_t type;
    uint64_t body, end;
};
struct Assoc {
    uint32_t item, index;
    bool essential;
};
struct Ref {  // dimg: a derived image and its inputs in order
    uint32_t from;
    std::vector<uint32_t> to;
};

enum { MAX_ITEMS = 16384, MAX_TILES = 4096 };

struct Msg {
    char* p;
    int n;
    explicit Msg(char* buf) : p(buf), n(0) { p[0] = 0; }
    Msg& s(const char* t) {
        while (*t && n < 126) p[n++] = *t++;
        p[n] = 0;
        return *this;
    }
    Msg& u(uint64_t v) {
        char t[24];
        int k = 0;
        do t[k++] = static_cast<char>('0' + v % 10);
        while ((v /= 10) != 0);
        while (k && n < 126) p[n++] = t[--k];
        p[n] = 0;
        return *this;
    }
    Msg& fourcc(uint32_t v) {
        for (int i = 3; i >= 0 && n < 126; i--) {
            const int c = static_cast<int>((v >> (8 * i)) & 255);
            p[n++] = (c >= 32 && c < 127 && c != '\'') ? static_cast<char>(c) : '?';
        }
        p[n] = 0;
        return *this;
    }
};

class Demux {
public:
    Demux(const uint8_t* d, uint64_t n, HeifResult& r) : d_(d), n_(n), r_(r) {}
    int run();

private:
    const uint8_t* d_;
    uint64_t n_;
    HeifResult& r_;
    std::vector<Item> items_;
    std::vector<Prop> props_;
    std::vector<Assoc> assoc_;
    std::vector<Ref> refs_;
    bool have_hdlr_ = false, have_pitm_ = false, have_idat_ = false;
    uint32_t primary_ = 0;
    uint64_t idat_body_ = 0, idat_end_ = 0;
    uint64_t spent_ = 0;  // bytes copied so far, against what a real file of this size could need

    int fail(int code, const char* text) {
        r_.error = code;
        Msg(r_.message).s(text);
        return code;
    }
    int malformed() { return fail(H2J_HEIF_MALFORMED, "HEIF: truncated or malformed box structure"); }
    int data_outside() { return fail(H2J_HEIF_DATA, "HEIF: item data outside the file"); }
    bool charge(uint64_t bytes) {
        spent_ += bytes;
        return spent_ <= 8 * n_ + (1u << 20);
    }
    Item* item(uint32_t id) {
        for (Item& it : items_)
            if (it.id == id) return &it;
        return nullptr;
    }
    Item* item_or_new(uint32_t id) {
        Item* it = item(id);
        if (it || items_.size() >= MAX_ITEMS) return it;
        Item fresh;
        fresh.id = id;
        fresh.type = 0;
        fresh.located = false;
        fresh.method = fresh.dref = 0;
        fresh.base = 0;
        items_.push_back(fresh);
        return &items_.back();
    }
    static bool known_property(uint32_t t) {
        return t == cc4('h', 'v', 'c', 'C') || t == cc4('a', 'v', 'c', 'C') || t == cc4('i', 's', 'p', 'e') ||
               t == cc4('i', 'r', 'o', 't') || t == cc4('i', 'm', 'i', 'r') || t == cc4('c', 'o', 'l', 'r') ||
               t == cc4('p', 'i', 'x', 'i') || t == cc4('c', 'l', 'a', 'p');
    }

    bool read_meta(const Box& meta);
    bool read_iinf(const Box& b);
    bool read_iloc(const Box& b);
    bool read_iref(const Box& b);
    bool read_iprp(const Box& b);
    bool read_ipma(const Box& b);
    int item_bytes(const Item& it, std::vector<uint8_t>& out);
    int check_properties(const Item& it, const Prop** config, bool orient);
    bool emit_nal(const uint8_t* p, uint64_t len);
    int emit_hvcc(const Prop& c, int* length_size);
    int emit_avcc(const Prop& c, int* length_size);
    int emit_item(const Item& it);
    int emit_grid(const Item& it);
};

bool Demux::read_iinf(const Box& b) {
    Rd r(d_, b.body, b.end);
    const uint64_t vf = r.be(4);
    r.skip((vf >> 24) == 0 ? 2 : 4);  // entry_count: the entries are walked as boxes instead
    Box e;
    while (next_box(r, e)) {
        if (e.type != cc4('i', 'n', 'f', 'e')) continue;
        Rd q(d_, e.body, e.end);
        const uint32_t ver = static_cast<uint32_t>(q.be(4) >> 24);
        if (ver < 2) continue;  // (no item type before version 2: such an item is never chosen)
        const uint32_t id = static_cast<uint32_t>(q.be(ver == 2 ? 2 : 4));
        q.skip(2);  // item_protection_index
        const uint32_t type = static_cast<uint32_t>(q.be(4));
        if (q.bad) return false;
        Item* it = item_or_new(id);
        if (!it) return false;
        it->type = type;
    }
    return !r.bad;
}

bool Demux::read_iloc(const Box& b) {
    Rd r(d_, b.body, b.end);
    const uint32_t ver = static_cast<uint32_t>(r.be(4) >> 24);
    const uint32_t s0 = static_cast<uint32_t>(r.be(1)), s1 = static_cast<uint32_t>(r.be(1));
    const int off_size = s0 >> 4, len_size = s0 & 15, base_size = s1 >> 4, idx_size = (ver == 1 || ver == 2) ? (s1 & 15) : 0;
    auto ok = [](int s) { return s == 0 || s == 4 || s == 8; };
    if (r.bad || ver > 2 || !ok(off_size) || !ok(len_size) || !ok(base_size) || !ok(idx_size)) return false;
    const uint64_t count = r.be(ver < 2 ? 2 : 4);
    for (uint64_t i = 0; i < count; i++) {
        const uint32_t id = static_cast<uint32_t>(r.be(ver < 2 ? 2 : 4));
        const uint32_t method = (ver == 1 || ver == 2) ? static_cast<uint32_t>(r.be(2) & 15) : 0;
        const uint32_t dref = static_cast<uint32_t>(r.be(2));
        const uint64_t base = r.be(base_size);
        const uint64_t nx = r.be(2);
        if (r.bad) return false;
        // the extent list is bounded by the bytes it occupies before one entry is stored: nx entries of `width`
        // bytes must fit what is left of the box, and entries of no width at all (every size nibble 0) can only
        // say "the whole source" once
        const uint64_t width = static_cast<uint64_t>(idx_size + off_size + len_size);
        if (width == 0 ? nx > 1 : nx > r.left() / width) return false;
        Item* it = item_or_new(id);
        if (!it) return false;
        it->located = true;
        it->method = method;
        it->dref = dref;
        it->base = base;
        it->ext.clear();
        for (uint64_t x = 0; x < nx; x++) {
            r.skip(idx_size);
            Extent e;
            e.off = r.be(off_size);
            e.len = r.be(len_size);
            if (r.bad) return false;
            it->ext.push_back(e);
        }
    }
    return !r.bad;
}

bool Demux::read_iref(const Box& b) {
    Rd r(d_, b.body, b.end);
    const uint32_t ver = static_cast<uint32_t>(r.be(4) >> 24);
    if (r.bad || ver > 1) return false;
    Box e;
    while (next_box(r, e)) {
        if (e.type != cc4('d', 'i', 'm', 'g')) continue;  // thmb, auxl, cdsc...: not followed
        Rd q(d_, e.body, e.end);
        Ref ref;
        ref.from = static_cast<uint32_t>(q.be(ver ? 4 : 2));
        const uint64_t cnt = q.be(2);
        for (uint64_t i = 0; i < cnt; i++) {
            const uint32_t to = static_cast<uint32_t>(q.be(ver ? 4 : 2));
            if (q.bad) return false;
            ref.to.push_back(to);
        }
        if (q.bad) return false;
        refs_.push_back(ref);
    }
    return !r.bad;
}

bool Demux::read_ipma(const Box& b) {
    Rd r(d_, b.body, b.end);
    const uint64_t vf = r.be(4);
    const uint32_t ver = static_cast<uint32_t>(vf >> 24);
    const bool wide = (vf & 1) != 0;
    const uint64_t count = r.be(4);
    for (uint64_t i = 0; i < count; i++) {
        const uint32_t id = static_cast<uint32_t>(r.be(ver < 1 ? 2 : 4));
        const uint64_t na = r.be(1);
        if (r.bad) return false;  // (before the next entry: a count past the box must not be walked to its end)
        for (uint64_t a = 0; a < na; a++) {
            const uint32_t v = static_cast<uint32_t>(r.be(wide ? 2 : 1));
            if (r.bad) return false;
            Assoc as;
            as.item = id;
            as.essential = wide ? (v >> 15) != 0 : (v >> 7) != 0;
            as.index = wide ? (v & 0x7FFF) : (v & 0x7F);
            assoc_.push_back(as);
        }
    }
    return !r.bad;
}

bool Demux::read_iprp(const Box& b) {
    Rd r(d_, b.body, b.end);
    Box c;
    while (next_box(r, c)) {
        if (c.type == cc4('i', 'p', 'c', 'o')) {
            Rd q(d_, c.body, c.end);
            Box p;
            while (next_box(q, p)) {
                Prop pr;
                pr.type = p.type;
                pr.body = p.body;
                pr.end = p.end;
                props_.push_back(pr);
            }
            if (q.bad) return false;
        } else if (c.type == cc4('i', 'p', 'm', 'a')) {
            if (!read_ipma(c)) return false;
        }
    }
    return !r.bad;
}

bool Demux::read_meta(const Box& meta) {
    Rd r(d_, meta.body, meta.end);
    r.skip(4);  // FullBox version and flags
    Box b;
    while (next_box(r, b)) {
        if (b.type == cc4('h', 'd', 'l', 'r')) {
            Rd q(d_, b.body, b.end);
            q.skip(8);
            const uint32_t handler = static_cast<uint32_t>(q.be(4));
            if (q.bad || handler != cc4('p', 'i', 'c', 't')) return false;
            have_hdlr_ = true;
        } else if (b.type == cc4('p', 'i', 't', 'm')) {
            Rd q(d_, b.body, b.end);
            const uint32_t ver = static_cast<uint32_t>(q.be(4) >> 24);
            primary_ = static_cast<uint32_t>(q.be(ver == 0 ? 2 : 4));
            if (q.bad || ver > 1) return false;
            have_pitm_ = true;
        } else if (b.type == cc4('i', 'i', 'n', 'f')) {
            if (!read_iinf(b)) return false;
        } else if (b.type == cc4('i', 'l', 'o', 'c')) {
            if (!read_iloc(b)) return false;
        } else if (b.type == cc4('i', 'd', 'a', 't')) {
            idat_body_ = b.body;
            idat_end_ = b.end;
            have_idat_ = true;
        } else if (b.type == cc4('i', 'r', 'e', 'f')) {
            if (!read_iref(b)) return false;
        } else if (b.type == cc4('i', 'p', 'r', 'p')) {
            if (!read_iprp(b)) return false;
        }
    }
    return !r.bad && have_hdlr_;
}

// the item's extents concatenated (construction method 0: file offsets; 1: offsets into idat)
int Demux::item_bytes(const Item& it, std::vector<uint8_t>& out) {
    out.clear();
    if (!it.located || it.dref != 0 || it.method > 1 || it.ext.empty() || (it.method == 1 && !have_idat_)) return data_outside();
    const uint64_t sb = it.method == 1 ? idat_body_ : 0, se = it.method == 1 ? idat_end_ : n_;
    const uint64_t srclen = se - sb;
    for (const Extent& e : it.ext) {
        if (it.base > ~static_cast<uint64_t>(0) - e.off) return data_outside();
        const uint64_t off = it.base + e.off;
        if (off > srclen) return data_outside();
        const uint64_t len = e.len ? e.len : srclen - off;  // (length 0: to the end of the source)
        if (len > srclen - off) return data_outside();
        if (!charge(len)) return data_outside();
        out.insert(out.end(), d_ + sb + off, d_ + sb + off + len);
        HeifSpan sp;
        sp.off = sb + off;
        sp.len = len;
        r_.spans.push_back(sp);
    }
    if (out.empty()) return data_outside();
    return 0;
}

// The properties ipma associates with the item, in its order: an essential one of a type this reader does not know
// fails the item (ISO/IEC 23008-12 6.5.1); clap is known and ignored (the whole picture is delivered, see DESIGN.md
// "HEIF input").  *config: the item's hvcC / avcC.  orient: compose the irot / imir into r_.orient
int Demux::check_properties(const Item& it, const Prop** config, bool orient) {
    *config = nullptr;
    for (const Assoc& a : assoc_) {
        if (a.item != it.id || a.index == 0) continue;
        if (a.index > props_.size()) return malformed();
        const Prop& p = props_[a.index - 1];
        if (!known_property(p.type)) {
            if (!a.essential) continue;
            r_.error = H2J_HEIF_UNSUPPORTED;
            Msg(r_.message).s("HEIF: essential property '").fourcc(p.type).s("' unsupported");
            return r_.error;
        }
        if ((p.type == cc4('h', 'v', 'c', 'C') || p.type == cc4('a', 'v', 'c', 'C')) && !*config) *config = &p;
        if (p.type == cc4('c', 'o', 'l', 'r') && !r_.nclx) {
            // the first nclx met: the primary item's properties are walked first, a grid's tiles' after the grid's own.
            // A colr that is short or of another type changes nothing, as it never did
            Rd c(d_, p.body, p.end);
            const uint32_t kind = static_cast<uint32_t>(c.be(4));
            const int pri = static_cast<int>(c.be(2)), trc = static_cast<int>(c.be(2)), mat = static_cast<int>(c.be(2));
            const int full = static_cast<int>(c.be(1) >> 7);
            if (!c.bad && kind == cc4('n', 'c', 'l', 'x')) {
                r_.nclx = true;
                r_.colour[0] = pri;
                r_.colour[1] = trc;
                r_.colour[2] = mat;
                r_.colour[3] = full;
            }
        }
        if (!orient) continue;
        Rd q(d_, p.body, p.end);
        if (p.type == cc4('i', 'r', 'o', 't')) {
            static const int kRot[4] = {1, 8, 3, 6};  // angle x 90 degrees anticlockwise
            const int angle = static_cast<int>(q.be(1) & 3);
            if (q.bad) return malformed();
            r_.orient = heif_compose_orient(r_.orient, kRot[angle]);
        } else if (p.type == cc4('i', 'm', 'i', 'r')) {
            const int axis = static_cast<int>(q.be(1) & 1);  // 0: vertical axis (left-right mirror), 1: horizontal axis
            if (q.bad) return malformed();
            r_.orient = heif_compose_orient(r_.orient, axis ? 4 : 2);
        }
    }
    return 0;
}

bool Demux::emit_nal(const uint8_t* p, uint64_t len) {
    if (!charge(len + 4)) return false;
    static const uint8_t kStart[4] = {0, 0, 0, 1};
    r_.bytes.insert(r_.bytes.end(), kStart, kStart + 4);
    r_.bytes.insert(r_.bytes.end(), p, p + len);
    return true;
}

// HEVCDecoderConfigurationRecord (ISO/IEC 14496-15 8.3.3.1): the arrays' NAL units as VPS, SPS, PPS, prefix SEI
int Demux::emit_hvcc(const Prop& c, int* length_size) {
    static const int kOrder[4] = {32, 33, 34, 39};
    for (int want : kOrder) {
        Rd q(d_, c.body, c.end);
        q.skip(21);
        *length_size = static_cast<int>(q.be(1) & 3) + 1;
        const uint64_t arrays = q.be(1);
        for (uint64_t a = 0; a < arrays; a++) {
            const int type = static_cast<int>(q.be(1) & 63);
            const uint64_t nn = q.be(2);
            for (uint64_t i = 0; i < nn; i++) {
                const uint64_t len = q.be(2);
                if (q.bad || q.left() < len) return malformed();
                if (type == want && len && !emit_nal(d_ + q.pos, len)) return data_outside();
                q.skip(len);
            }
        }
        if (q.bad) return malformed();
    }
    return 0;
}

// AVCDecoderConfigurationRecord (ISO/IEC 14496-15 5.3.3.1): SPS, then PPS
int Demux::emit_avcc(const Prop& c, int* length_size) {
    Rd q(d_, c.body, c.end);
    q.skip(4);
    *length_size = static_cast<int>(q.be(1) & 3) + 1;
    for (int set = 0; set < 2; set++) {
        const uint64_t nn = q.be(1) & (set == 0 ? 31 : 255);
        for (uint64_t i = 0; i < nn; i++) {
            const uint64_t len = q.be(2);
            if (q.bad || q.left() < len) return malformed();
            if (len && !emit_nal(d_ + q.pos, len)) return data_outside();
            q.skip(len);
        }
    }
    return q.bad ? malformed() : 0;
}

// one coded item appended to r_.bytes as an Annex-B stream
int Demux::emit_item(const Item& it) {
    const Prop* config = nullptr;
    const int pe = check_properties(it, &config, false);
    if (pe) return pe;
    const bool hevc = it.type == cc4('h', 'v', 'c', '1');
    if (!config || config->type != (hevc ? cc4('h', 'v', 'c', 'C') : cc4('a', 'v', 'c', 'C')))
        return fail(H2J_HEIF_NO_CONFIG, "HEIF: item has no decoder configuration");
    int ls = 4;
    const int ce = hevc ? emit_hvcc(*config, &ls) : emit_avcc(*config, &ls);
    if (ce) return ce;
    std::vector<uint8_t> payload;
    const int be = item_bytes(it, payload);
    if (be) return be;
    Rd q(payload.data(), 0, payload.size());
    while (q.left() > 0) {
        const uint64_t len = q.be(ls);
        if (q.bad || len == 0 || q.left() < len) return fail(H2J_HEIF_MALFORMED, "HEIF: NAL unit lengths run past the item");
        if (!emit_nal(payload.data() + q.pos, len)) return data_outside();
        q.skip(len);
    }
    return 0;
}

int Demux::emit_grid(const Item& it) {
    std::vector<uint8_t> g;
    const int be = item_bytes(it, g);
    if (be) return be;
    Rd q(g.data(), 0, g.size());
    const uint64_t version = q.be(1), flags = q.be(1);
    const uint64_t rows = q.be(1) + 1, cols = q.be(1) + 1;
    const uint64_t w = q.be((flags & 1) ? 4 : 2), h = q.be((flags & 1) ? 4 : 2);
    if (q.bad || version != 0 || w == 0 || h == 0 || w > (1u << 30) || h > (1u << 30)) return malformed();
    const Ref* ref = nullptr;
    for (const Ref& r : refs_)
        if (r.from == it.id && !ref) ref = &r;
    const uint64_t have = ref ? ref->to.size() : 0;
    if (have != rows * cols) {
        r_.error = H2J_HEIF_GRID;
        Msg(r_.message).s("HEIF: grid references ").u(have).s(" items, needs ").u(rows).s(" \xC3\x97 ").u(cols);
        return r_.error;
    }
    if (rows * cols > MAX_TILES) {
        r_.error = H2J_HEIF_GRID;
        Msg(r_.message).s("HEIF: grid of ").u(rows * cols).s(" tiles exceeds ").u(MAX_TILES);
        return r_.error;
    }
    r_.grid = true;
    r_.rows = static_cast<int>(rows);
    r_.cols = static_cast<int>(cols);
    r_.out_w = static_cast<int>(w);
    r_.out_h = static_cast<int>(h);
    for (uint32_t id : ref->to) {
        const Item* t = item(id);
        if (!t) return malformed();
        if (t->type == cc4('a', 'v', 'c', '1')) return fail(H2J_HEIF_UNSUPPORTED, "HEIF: grid of AVC tiles unsupported");
        if (t->type != cc4('h', 'v', 'c', '1')) {
            r_.error = H2J_HEIF_UNSUPPORTED;
            Msg(r_.message).s("HEIF: grid tile type '").fourcc(t->type).s("' unsupported");
            return r_.error;
        }
        const int e = emit_item(*t);
        if (e) return e;
        r_.tile_off.push_back(r_.bytes.size());
    }
    return 0;
}

int Demux::run() {
    Rd top(d_, 0, n_);
    Box b;
    bool found = false;
    while (!found && next_box(top, b)) found = b.type == cc4('m', 'e', 't', 'a');
    if (!found) return malformed();
    if (!read_meta(b)) return malformed();
    if (!have_pitm_) return fail(H2J_HEIF_NO_PRIMARY, "HEIF: no primary item");
    const Item* it = item(primary_);
    if (!it || it->type == 0) return fail(H2J_HEIF_NO_PRIMARY, "HEIF: no primary item");
    const bool grid = it->type == cc4('g', 'r', 'i', 'd');
    if (!grid && it->type != cc4('h', 'v', 'c', '1') && it->type != cc4('a', 'v', 'c', '1')) {
        r_.error = H2J_HEIF_UNSUPPORTED;
        Msg(r_.message).s("HEIF: primary item type '").fourcc(it->type).s("' unsupported");
        return r_.error;
    }
    const Prop* unused = nullptr;
    const int pe = check_properties(*it, &unused, true);
    if (pe) return pe;
    if (r_.orient == 1) r_.orient = 0;
    r_.codec = it->type == cc4('a', 'v', 'c', '1') ? 264 : 265;
    r_.tile_off.push_back(0);
    if (grid) return emit_grid(*it);
    const int e = emit_item(*it);
    if (e) return e;
    r_.tile_off.push_back(r_.bytes.size());
    return 0;
}

}  // namespace

bool is_heif(const uint8_t* d, size_t n) {
    if (!d || n < 16) return false;
    if (d[4] != 'f' || d[5] != 't' || d[6] != 'y' || d[7] != 'p') return false;
    const uint64_t size = (static_cast<uint64_t>(d[0]) << 24) | (static_cast<uint64_t>(d[1]) << 16) | (static_cast<uint64_t>(d[2]) << 8) | d[3];
    if (size < 16 || size > 4096 || (size & 3)) return false;
    static const uint32_t kBrands[7] = {cc4('h', 'e', 'i', 'c'), cc4('h', 'e', 'i', 'x'), cc4('h', 'e', 'v', 'c'), cc4('h', 'e', 'v', 'x'),
                                        cc4('m', 'i', 'f', '1'), cc4('m', 's', 'f', '1'), cc4('a', 'v', 'c', 'i')};
    const uint64_t end = size < n ? size : n;
    for (uint64_t at = 8; at + 4 <= end; at += 4) {
        if (at == 12) continue;  // minor_version
        const uint32_t b = cc4(static_cast<char>(d[at]), static_cast<char>(d[at + 1]), static_cast<char>(d[at + 2]), static_cast<char>(d[at + 3]));
        for (uint32_t k : kBrands)
            if (b == k) return true;
    }
    return false;
}

int heif_compose_orient(int first, int then) {
    // an orientation as (transpose, then mirror left-right, then mirror top-bottom) of the decoded picture
    static const uint8_t kT[9] = {0, 0, 0, 0, 0, 1, 1, 1, 1}, kX[9] = {0, 0, 1, 1, 0, 0, 1, 1, 0}, kY[9] = {0, 0, 0, 1, 1, 0, 0, 1, 1};
    static const uint8_t kCode[2][2][2] = {{{1, 4}, {2, 3}}, {{5, 8}, {6, 7}}};  // [transpose][left-right][top-bottom]
    if (first < 0 || first > 8 || then < 0 || then > 8) return 0;
    const int t = kT[first] ^ kT[then];
    // a transpose moves a left-right mirror made before it to top-bottom, and the reverse
    const int x = (kT[then] ? kY[first] : kX[first]) ^ kX[then];
    const int y = (kT[then] ? kX[first] : kY[first]) ^ kY[then];
    const int code = kCode[t][x][y];
    return code == 1 ? 0 : code;
}

int heif_demux(const uint8_t* d, size_t n, HeifResult& r) {
    r = HeifResult();
    if (!is_heif(d, n)) {
        r.error = H2J_HEIF_MALFORMED;
        Msg(r.message).s("HEIF: truncated or malformed box structure");
        return r.error;
    }
    Demux dm(d, n, r);
    const int e = dm.run();
    if (e) {
        r.bytes.clear();
        r.tile_off.clear();
    }
    return e;
}

}  // namespace h2j
