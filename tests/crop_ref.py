"""Model of the window and cover rule (include/h2j.h "Crop and cover", h2j_crop_window), restated from
the documented rule in plain Python integers: no numpy, no engine.

A rendition of a cropped W x H picture may name a window (x, y, w, h) in luma samples; w, h 0 mean "to the
right / bottom edge".  cover=(bw, bh) shrinks the window to the box's aspect, centred, and sizes it as a
stretch fit does.  The remaining options (scale, max_dim, fit, stretch) act on the window as they act on a
picture of its size.  `resolve` returns None where the engine fails the rendition (H2J_ERR_OUT_OPTS).
"""

STRETCH, COVER = 1, 2
RESAMPLE = 4  # mode of an output K3r makes (h2j_jobs.h H2J_SCALE_RESAMPLE)


def scaled_size(w, h, k):
    s = 2 << k
    return (2 * -(-w // s), 2 * -(-h // s)) if k else (w, h)


def fit_size(w, h, fw, fh, stretch):
    bw = min(fw, w) if fw else w
    bh = min(fh, h) if fh else h
    if stretch:
        return 2 * (bw // 2), 2 * (bh // 2)
    if bw * h <= bh * w:
        ow = 2 * (bw // 2)
        return ow, 2 * max(1, (h * ow) // (2 * w))
    oh = 2 * (bh // 2)
    return 2 * max(1, (w * oh) // (2 * h)), oh


def options_valid(scale, max_dim, fw, fh, flags, crop, reserved=(0, 0, 0)):
    """What the engine can say before it knows the picture's size."""
    if not 0 <= scale <= 3 or max_dim < 0 or any(reserved):
        return False
    if any(c < 0 or c % 2 for c in crop):
        return False
    if flags & ~(STRETCH | COVER):
        return False
    box_ok = all(f == 0 or 2 <= f <= 65535 for f in (fw, fh))
    if flags & COVER:
        return flags == COVER and box_ok and fw >= 2 and fh >= 2 and scale == 0 and max_dim == 0
    if not box_ok or (flags & STRETCH and fw == 0 and fh == 0):
        return False
    return not ((fw or fh) and (scale or max_dim))


def resolve(W, H, scale=0, max_dim=0, fw=0, fh=0, flags=0, crop=(0, 0, 0, 0), reserved=(0, 0, 0)):
    """((x, y, w, h), (ow, oh), mode) or None.  mode: 0 unscaled, 1..3 K3s at that scale, 4 K3r."""
    if W < 2 or H < 2 or W > 65536 or H > 65536 or W % 2 or H % 2:
        return None
    if not options_valid(scale, max_dim, fw, fh, flags, crop, reserved):
        return None
    x, y, w, h = crop
    w = w or W - x
    h = h or H - y
    if w < 2 or h < 2 or x + w > W or y + h > H:
        return None
    if flags & COVER:
        if w * fh >= h * fw:
            cw, ch = min(max(2 * ((h * fw) // (2 * fh)), 2), w), h
        else:
            cw, ch = w, min(max(2 * ((w * fh) // (2 * fw)), 2), h)
        x += 2 * ((w - cw) // 4)
        y += 2 * ((h - ch) // 4)
        w, h = cw, ch
        flags = STRETCH
    k = scale
    if max_dim > 0:
        while k < 3 and max(scaled_size(w, h, k)) > max_dim:
            k += 1
    if not (fw or fh):
        return (x, y, w, h), scaled_size(w, h, k), k
    ow, oh = fit_size(w, h, fw, fh, bool(flags & STRETCH))
    if (ow, oh) == (w, h):
        return (x, y, w, h), (w, h), 0
    for k in (1, 2, 3):
        if (ow << k, oh << k) == (w, h):
            return (x, y, w, h), (ow, oh), k
    return (x, y, w, h), (ow, oh), RESAMPLE


def spec_fields(spec):
    """A rendition spec of the tests -- an int (scale) or a dict with scale, max_dim, fit, stretch, crop,
    cover -- as resolve's keyword arguments."""
    if isinstance(spec, int):
        return dict(scale=spec)
    fw, fh = spec.get("cover") or spec.get("fit") or (0, 0)
    flags = (COVER if "cover" in spec else 0) | (STRETCH if spec.get("stretch") else 0)
    return dict(scale=spec.get("scale", 0), max_dim=spec.get("max_dim", 0), fw=fw or 0, fh=fh or 0, flags=flags,
                crop=tuple(spec.get("crop") or (0, 0, 0, 0)))


def window_planes(y, u, v, win):
    """The window's samples of cropped planes (any 2-D sliceable arrays): the one definition."""
    x, yy, w, h = win
    return (y[yy:yy + h, x:x + w], u[yy // 2:(yy + h) // 2, x // 2:(x + w) // 2],
            v[yy // 2:(yy + h) // 2, x // 2:(x + w) // 2])
