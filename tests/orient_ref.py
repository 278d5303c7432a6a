"""Model of oriented output (include/h2j.h "Orientation", DESIGN.md "Orientation (K3o)"): no engine.

An orientation is 0..8; 0 and 1 mean "as decoded", 2..8 are the EXIF / TIFF orientation numbers.  The
oriented picture is the picture: every other option acts on the oriented planes, so expected planes and
files come from the existing models (scale_ref, resize_ref, crop_ref, oracle_py) on `orient_planes`.

The display orientation SEI (payload type 47; H.264 D.2.27, H.265 D.3.17) says: flip, then rotate
anticlockwise.  `sei_orient` derives the EXIF number of a (hor_flip, ver_flip, quarter turns) triple by
applying those steps to an asymmetric array and finding which of the eight codes gives the same array --
independently of the table the host keeps.  `insert_sei` builds such an SEI NAL unit bit by bit and puts it
in front of the first slice of a golden stream.
"""
import numpy as np

import crop_ref

AUTO = -1


def orient_plane(p, o):
    """The oriented plane of a cropped plane p (H x W) -- the table of include/h2j.h."""
    if o in (0, 1):
        return p
    if o == 2:
        return p[:, ::-1]
    if o == 3:
        return p[::-1, ::-1]
    if o == 4:
        return p[::-1, :]
    if o == 5:
        return p.T
    if o == 6:
        return np.rot90(p, -1)
    if o == 7:
        return p[::-1, ::-1].T
    if o == 8:
        return np.rot90(p, 1)
    raise ValueError(f"orientation {o}")


def orient_planes(y, u, v, o):
    return tuple(np.ascontiguousarray(orient_plane(p, o)) for p in (y, u, v))


def inverse(o):
    """The orientation that undoes o."""
    return {0: 0, 1: 0, 2: 2, 3: 3, 4: 4, 5: 5, 6: 8, 7: 7, 8: 6}[o]


_PROBE = np.arange(3 * 5).reshape(3, 5)  # no symmetry: the eight oriented arrays all differ


def sei_orient(hor, ver, k):
    """The EXIF number of: hor_flip, then ver_flip, then k quarter turns anticlockwise (0: none of it)."""
    p = _PROBE
    if hor:
        p = p[:, ::-1]
    if ver:
        p = p[::-1, :]
    p = np.rot90(p, k)
    hits = [o for o in (0, 2, 3, 4, 5, 6, 7, 8) if orient_plane(_PROBE, o).shape == p.shape and (orient_plane(_PROBE, o) == p).all()]
    assert len(hits) == 1, (hor, ver, k, hits)
    return hits[0]


def resolve_orient(orient, sei=0):
    """The orientation (0, 2..8) a rendition's `orient` names for a picture whose SEI says `sei`; None: invalid."""
    if not -1 <= orient <= 8 or not 0 <= sei <= 8:
        return None
    o = sei if orient == AUTO else orient
    return 0 if o == 1 else o


def resolve(W, H, orient=0, sei=0, reserved=(0, 0, 0, 0, 0, 0), **kw):
    """crop_ref.resolve on the oriented size of a decoded W x H picture: ((x, y, w, h), (ow, oh), mode, orientation)
    with the window in the oriented picture, or None where the engine fails the rendition."""
    o = resolve_orient(orient, sei)
    if o is None or any(reserved):
        return None
    r = crop_ref.resolve(H, W, **kw) if o >= 5 else crop_ref.resolve(W, H, **kw)
    return None if r is None else r + (o,)


def spec_fields(spec):
    """crop_ref.spec_fields with the orient key ("auto": AUTO)."""
    if isinstance(spec, int):
        return dict(scale=spec)
    kw = crop_ref.spec_fields({k: v for k, v in spec.items() if k != "orient"})
    o = spec.get("orient", 0)
    kw["orient"] = AUTO if o == "auto" else o
    return kw


# ---------------------------------------------------------------- SEI NAL units
class Bits:
    def __init__(self):
        self.b = []

    def u(self, n, v):
        self.b += [(v >> (n - 1 - i)) & 1 for i in range(n)]
        return self

    def ue(self, v):
        n = (v + 1).bit_length()
        return self.u(n - 1, 0).u(n, v + 1)

    def bytes(self):
        assert len(self.b) % 8 == 0
        return bytes(int("".join(map(str, self.b[i:i + 8])), 2) for i in range(0, len(self.b), 8))


def orientation_payload(codec, hor=0, ver=0, rotation=0, cancel=0):
    """The display_orientation payload bytes (payload type 47), with the payload alignment bits."""
    b = Bits().u(1, cancel)
    if not cancel:
        b.u(1, hor).u(1, ver).u(16, rotation)
        if codec == 265:
            b.u(1, 1)  # display_orientation_persistence_flag
        else:
            b.ue(1).u(1, 0)  # display_orientation_repetition_period, display_orientation_extension_flag
    if len(b.b) % 8:  # payload_bit_equal_to_one, then zeros to the byte boundary
        b.u(1, 1)
        b.u(-len(b.b) % 8, 0)
    return b.bytes()


def sei_message(ptype, payload, size=None):
    """One sei_message: type and size with their 0xFF extension bytes, then the payload (size: a lie about it)."""
    size = len(payload) if size is None else size
    out = b""
    for v in (ptype, size):
        out += b"\xff" * (v // 255) + bytes([v % 255])
    return out + payload


def escape(rbsp):
    """Emulation prevention: 00 00 0x (x <= 3) gets a 03 in front of its third byte."""
    out, zeros = bytearray(), 0
    for c in rbsp:
        if zeros >= 2 and c <= 3:
            out.append(3)
            zeros = 0
        out.append(c)
        zeros = zeros + 1 if c == 0 else 0
    return bytes(out)


def sei_nal(codec, messages, trailing=True):
    """An SEI NAL unit (start code included) of the concatenated messages, with the RBSP trailing bits."""
    hdr = bytes([39 << 1, 1]) if codec == 265 else bytes([6])  # PREFIX_SEI_NUT, nuh_temporal_id_plus1 1 / SEI
    rbsp = b"".join(messages) + (b"\x80" if trailing else b"")
    return b"\x00\x00\x00\x01" + hdr + escape(rbsp)


def nal_spans(stream):
    """(start of the start code, start of the NAL header, end) of every NAL unit."""
    starts, i = [], 0
    while True:
        i = stream.find(b"\x00\x00\x01", i)
        if i < 0:
            break
        starts.append(i)
        i += 3
    spans = []
    for k, s in enumerate(starts):
        e = starts[k + 1] if k + 1 < len(starts) else len(stream)
        s0 = s - 1 if s > 0 and stream[s - 1] == 0 else s
        spans.append((s0, s + 3, e))
    # a 4-byte start code's leading zero belongs to the NAL that follows, not to the one before
    return [(s0, h, (spans[k + 1][0] if k + 1 < len(spans) else e)) for k, (s0, h, e) in enumerate(spans)]


def is_vcl(codec, stream, h):
    if codec == 265:
        t = (stream[h] >> 1) & 63
        return t <= 21 and not 10 <= t <= 15
    return (stream[h] & 31) in (1, 5)


def insert_nal(stream, codec, nal, after_first_slice=False):
    """The stream with `nal` in front of its first VCL NAL unit (or behind it)."""
    for s0, h, e in nal_spans(stream):
        if is_vcl(codec, stream, h):
            at = e if after_first_slice else s0
            return stream[:at] + nal + stream[at:]
    raise AssertionError("no slice in the stream")


def insert_sei(stream, codec, hor=0, ver=0, k=0, **kw):
    """The stream with a display orientation SEI (flips, k quarter turns anticlockwise) in front of its first slice."""
    return insert_nal(stream, codec, sei_nal(codec, [sei_message(47, orientation_payload(codec, hor, ver, (k & 3) << 14, **kw))]))
