"""An independent HEIF muxer: Annex-B streams in, HEIF bytes out (test infrastructure).

Writes the `meta`-box layouts the demuxer (csrc/host/heif.cpp) has to read, from the box syntax of ISO/IEC 14496-12
(box headers, FullBox, hdlr, pitm, iinf / infe, iloc, idat, iref) and ISO/IEC 23008-12 (iprp / ipco / ipma, ispe,
irot, imir, the ImageGrid payload) and the decoder configuration records of ISO/IEC 14496-15 (hvcC, avcC), restated
here without any HEIF library: none is available to check it against, so parity with a real encoder's HEIC is unpinned.

    mux([stream])                          one hvc1 item (codec=264: one avc1 item)
    mux(tiles, grid=(rows, cols, W, H))    a grid item over rows * cols hvc1 tile items in raster order

Knobs, each a variant of the syntax:
    iloc_version 0 | 1 | 2        offset_size, length_size 4 | 8      base_offset_size 0 | 4 | 8
    index_size 0 | 4 | 8 (iloc version 1, 2)      extents >= 1 (the item's payload in that many separate pieces)
    construction 0 | 1 (coded items: file offsets, or idat)      grid_construction 1 | 0 (the grid descriptor)
    infe_version 2 | 3    pitm_version 0 | 1    ipma_version 0 | 1    ipma_wide (15-bit property indices)
    grid32 (32-bit grid sizes)    largesize (64-bit box sizes on meta and mdat)    mdat_first
    thumb, aux (a thmb / auxl item beside the primary, listed before it)
    transforms, e.g. [("irot", 1), ("imir", 0)] in ipma order      nal_length_size 1 | 2 | 4
    essential_unknown (an essential property of unknown type on the primary)    clap (an essential clap)
    primary_type (another item type for the primary, e.g. b"av01")    no_pitm, no_config, drop_refs (rejections)
"""
import struct


def split_nals(stream: bytes):
    """NAL units of an Annex-B stream (start codes and trailing zero bytes dropped)."""
    out, i, n = [], 0, len(stream)
    starts = []
    while i + 3 <= n:
        if stream[i] == 0 and stream[i + 1] == 0 and stream[i + 2] == 1:
            starts.append(i + 3)
            i += 3
        else:
            i += 1
    for k, s in enumerate(starts):
        e = starts[k + 1] - 3 if k + 1 < len(starts) else n
        nal = stream[s:e].rstrip(b"\x00")
        if nal:
            out.append(nal)
    return out


def _type(nal, codec):
    return (nal[0] >> 1) & 63 if codec == 265 else nal[0] & 31


def config_and_payload(stream, codec, sei_in_config=True):
    """(configuration NAL units in record order, payload NAL units)"""
    nals = split_nals(stream)
    order = ([32, 33, 34] + ([39] if sei_in_config else [])) if codec == 265 else [7, 8]
    first_vcl = next(i for i, x in enumerate(nals) if (_type(x, codec) <= 21 if codec == 265 else _type(x, codec) in (1, 5)))
    cfg = [x for t in order for x in nals[:first_vcl] if _type(x, codec) == t]
    rest = [x for i, x in enumerate(nals) if i >= first_vcl or _type(x, codec) not in order]
    return cfg, rest


def expected_annexb(stream, codec=265, sei_in_config=True):
    """What the demuxer must give back for an item muxed from `stream`."""
    cfg, rest = config_and_payload(stream, codec, sei_in_config)
    return b"".join(b"\x00\x00\x00\x01" + x for x in cfg + rest)


def box(kind: bytes, payload: bytes, large=False) -> bytes:
    if large:
        return struct.pack(">I4sQ", 1, kind, 16 + len(payload)) + payload
    return struct.pack(">I4s", 8 + len(payload), kind) + payload


def fullbox(kind, version, flags, payload, large=False):
    return box(kind, struct.pack(">I", (version << 24) | flags) + payload, large)


def _uint(v, size):
    return v.to_bytes(size, "big") if size else b""


def hvcc(cfg, length_size):
    arrays = []
    for t in (32, 33, 34, 39):
        group = [x for x in cfg if _type(x, 265) == t]
        if group:
            arrays.append(bytes([0x80 | t]) + struct.pack(">H", len(group)) + b"".join(struct.pack(">H", len(x)) + x for x in group))
    head = bytes([1, 1]) + b"\x60\x00\x00\x00" + b"\x90\x00\x00\x00\x00\x00" + bytes([93]) + b"\xF0\x00" + bytes([0xFC, 0xFD, 0xF8, 0xF8]) + b"\x00\x00"
    head += bytes([0x0C | (length_size - 1)])
    assert len(head) == 22
    return box(b"hvcC", head + bytes([len(arrays)]) + b"".join(arrays))


def avcc(cfg, length_size):
    sps = [x for x in cfg if _type(x, 264) == 7]
    pps = [x for x in cfg if _type(x, 264) == 8]
    out = bytes([1]) + sps[0][1:4] + bytes([0xFC | (length_size - 1), 0xE0 | len(sps)])
    out += b"".join(struct.pack(">H", len(x)) + x for x in sps) + bytes([len(pps)]) + b"".join(struct.pack(">H", len(x)) + x for x in pps)
    return box(b"avcC", out)


def find_box(data: bytes, kind: bytes):
    """(offset, length) of the first top-level box of that type"""
    at = 0
    while at + 8 <= len(data):
        size, k = struct.unpack(">I4s", data[at:at + 8])
        if size == 1:
            size = struct.unpack(">Q", data[at + 8:at + 16])[0]
        elif size == 0:
            size = len(data) - at
        if k == kind:
            return at, size
        at += size
    raise KeyError(kind)


def mux(streams, codec=265, grid=None, brand=b"heic", iloc_version=0, offset_size=4, length_size=4, base_offset_size=0,
        index_size=0, extents=1, construction=0, grid_construction=1, infe_version=2, pitm_version=0, ipma_version=0,
        ipma_wide=False, grid32=False, largesize=False, mdat_first=False, thumb=False, aux=False, transforms=(),
        nal_length_size=4, essential_unknown=False, clap=False, primary_type=None, no_pitm=False, no_config=False,
        drop_refs=0, sei_in_config=True, tile_size=(0, 0), tile_codec=None):
    tile_codec = tile_codec or codec
    item_type = {265: b"hvc1", 264: b"avc1"}
    # ---- items: [id, type, payload bytes or None (no data), method]
    items, payloads = [], {}
    cfgs = []
    for s in streams:
        cfg, rest = config_and_payload(s, tile_codec, sei_in_config)
        cfgs.append(cfg)
        payloads[len(cfgs)] = b"".join(_uint(len(x), nal_length_size) + x for x in rest)
    T = len(streams)
    extra = []
    if thumb:
        extra.append((b"thmb", T + 2))
    if aux:
        extra.append((b"auxl", T + 3))
    primary = T + 1 if grid else 1
    for _, eid in extra:  # listed before the primary: a reader that takes the first item takes the wrong one
        items.append([eid, item_type[tile_codec], payloads[1], construction])
    for i in range(T):
        items.append([i + 1, item_type[tile_codec], payloads[i + 1], construction])
    if grid:
        rows, cols, W, H = grid
        fmt = ">BBBBII" if grid32 else ">BBBBHH"
        desc = struct.pack(fmt, 0, 1 if grid32 else 0, rows - 1, cols - 1, W, H)
        items.append([primary, b"grid", desc, grid_construction])
    if primary_type:
        for it in items:
            if it[0] == primary:
                it[1] = primary_type
    if iloc_version == 0 and any(it[3] == 1 for it in items):
        iloc_version = 1  # (version 0 has no construction method: idat needs version 1 or 2)
    # ---- properties (1-based indices in ipco order) and associations: item -> [(index, essential)]
    props, assoc = [], {}

    def prop(b):
        props.append(b)
        return len(props)

    distinct = {}
    for i, cfg in enumerate(cfgs):
        key = tuple(cfg)
        if key not in distinct and not no_config:
            distinct[key] = prop(hvcc(cfg, nal_length_size) if tile_codec == 265 else avcc(cfg, nal_length_size))
        assoc[i + 1] = ([(distinct[key], True)] if not no_config else [])
    ispe_tile = prop(fullbox(b"ispe", 0, 0, struct.pack(">II", *tile_size)))
    colr = prop(box(b"colr", b"nclx" + struct.pack(">HHHB", 1, 1, 1, 0x80)))
    pixi = prop(fullbox(b"pixi", 0, 0, bytes([3, 8, 8, 8])))
    for i in range(T):
        assoc[i + 1] += [(ispe_tile, False), (colr, False), (pixi, False)]
    for _, eid in extra:
        assoc[eid] = list(assoc[1]) + [(prop(box(b"auxC", b"urn:test\x00")), False)]
    if grid:
        assoc[primary] = [(prop(fullbox(b"ispe", 0, 0, struct.pack(">II", grid[2], grid[3]))), False)]
    assoc[primary].append((prop(box(b"zzzz", b"unknown property")), essential_unknown))
    if clap:
        assoc[primary].append((prop(box(b"clap", struct.pack(">IIIIiIiI", 2, 1, 2, 1, 0, 1, 0, 1))), True))
    for kind, value in transforms:
        assoc[primary].append((prop(box(kind.encode(), bytes([value]))), True))
    # ---- meta, built for given data positions
    refs = []
    if grid:
        refs.append((b"dimg", primary, list(range(1, T + 1))[:T - drop_refs]))
    for kind, eid in extra:
        refs.append((kind, eid, [primary]))
    idat_items = [it for it in items if it[3] == 1]
    idat_payload, idat_at = b"", {}
    for it in idat_items:
        idat_at[it[0]] = len(idat_payload)
        idat_payload += it[2] + b"\xA5\xA5\xA5"  # (a gap: items are not back to back)

    def pieces(data):
        k = min(extents, max(1, len(data)))
        cut = [len(data) * j // k for j in range(k + 1)]
        return [data[cut[j]:cut[j + 1]] for j in range(k)]

    mdat_payload, mdat_at = b"", {}
    for it in items:
        if it[3] == 0:
            mdat_at[it[0]] = []
            for piece in reversed(pieces(it[2])):  # (stored out of order, with gaps)
                mdat_payload += b"\x5A" * 5
                mdat_at[it[0]].insert(0, (len(mdat_payload), len(piece)))
                mdat_payload += piece

    def meta(mdat_body):
        idw = 2 if infe_version == 2 else 4
        hdlr = fullbox(b"hdlr", 0, 0, struct.pack(">I4s", 0, b"pict") + b"\x00" * 12 + b"\x00")
        pitm = b"" if no_pitm else fullbox(b"pitm", pitm_version, 0, _uint(primary, 2 if pitm_version == 0 else 4))
        infes = b"".join(fullbox(b"infe", infe_version, 1 if it[0] != primary and grid else 0,
                                 _uint(it[0], idw) + struct.pack(">H4s", 0, it[1]) + b"\x00") for it in items)
        iinf = fullbox(b"iinf", 0, 0, struct.pack(">H", len(items)) + infes)
        v = iloc_version
        body = bytes([(offset_size << 4) | length_size, (base_offset_size << 4) | (index_size if v in (1, 2) else 0)])
        body += _uint(len(items), 2 if v < 2 else 4)
        for it in items:
            method = it[3]
            assert method == 0 or v in (1, 2), "construction method 1 needs iloc version 1 or 2"
            ext = [(idat_at[it[0]], len(it[2]))] if method == 1 else [(mdat_body + o, n) for o, n in mdat_at[it[0]]]
            base = 0
            if base_offset_size:
                base = min(o for o, _ in ext)
                ext = [(o - base, n) for o, n in ext]
            body += _uint(it[0], 2 if v < 2 else 4)
            if v in (1, 2):
                body += struct.pack(">H", method)
            body += struct.pack(">H", 0) + _uint(base, base_offset_size) + struct.pack(">H", len(ext))
            for o, n in ext:
                if v in (1, 2):
                    body += _uint(0, index_size)
                body += _uint(o, offset_size) + _uint(n, length_size)
        iloc = fullbox(b"iloc", v, 0, body)
        idat = box(b"idat", idat_payload) if idat_items else b""
        iref = fullbox(b"iref", 0, 0, b"".join(box(k, struct.pack(">HH", f, len(to)) + b"".join(struct.pack(">H", t) for t in to))
                                               for k, f, to in refs)) if refs else b""
        entries = b""
        for iid in sorted(assoc):
            entries += _uint(iid, 2 if ipma_version < 1 else 4) + bytes([len(assoc[iid])])
            for idx, ess in assoc[iid]:
                entries += struct.pack(">H", (0x8000 if ess else 0) | idx) if ipma_wide else bytes([(0x80 if ess else 0) | idx])
        ipma = fullbox(b"ipma", ipma_version, 1 if ipma_wide else 0, struct.pack(">I", len(assoc)) + entries)
        iprp = box(b"iprp", box(b"ipco", b"".join(props)) + ipma)
        return fullbox(b"meta", 0, 0, hdlr + pitm + iinf + iloc + idat + iref + iprp, largesize)

    ftyp = box(b"ftyp", brand + struct.pack(">I", 0) + b"mif1" + brand)
    mhdr = 16 if largesize else 8
    if mdat_first:
        m = meta(len(ftyp) + mhdr)
        return ftyp + box(b"mdat", mdat_payload, largesize) + box(b"free", b"pad") + m
    m0 = meta(0)
    m = meta(len(ftyp) + len(m0) + mhdr)
    assert len(m) == len(m0)
    return ftyp + m + box(b"mdat", mdat_payload, largesize)
