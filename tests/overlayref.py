"""The text overlay's drawing rule in numpy, written from the rule's text, on the sample grid: masks of the whole
picture, no font-pixel neighbourhoods.  The font comes through mi355enc_overlay_glyph (host only).

All arithmetic is integer.  The rule works on the visible NV12 picture (w x h, both even); the coded-size surfaces follow by edge replication
(tests/util.py pad_planes), "as if the text had been in the picture before padding"."""
import numpy as np

from ceracoder_amd import enc as E

LEFT, CENTRE, RIGHT = 0, 1, 2
TOP, BOTTOM = 0, 2
MAX_TEXT = 255
DEFAULT = dict(halign=RIGHT, valign=TOP, xpad=16, ypad=16, scale=0, shaded_background=0)

_font = {}


def glyph(ch):
    """(16, 8) bool: the cell of byte `ch`; bytes outside 0x20 .. 0x7E draw as '?'"""
    if ch < 0x20 or ch > 0x7E:
        ch = ord("?")
    if ch not in _font:
        rows = E.overlay_glyph(ch)
        _font[ch] = ((rows[:, None] >> (7 - np.arange(8))[None, :]) & 1).astype(bool)
    return _font[ch]


def as_bytes(text):
    b = text.encode("latin-1") if isinstance(text, str) else bytes(text or b"")
    return b[:MAX_TEXT]


def auto_scale(h):
    return min(max(h // 540, 1), 8)


def masks(text, w, h, **style):
    """-> (T, O, B): bool (h, w) masks of the text samples, the outline and the box on the visible luma grid; None with no text or an invisible box"""
    st = dict(DEFAULT, **style)
    b = as_bytes(text)
    if not b:
        return None
    lines = b.split(b"\n")
    s = st["scale"] or auto_scale(h)
    cols = max(len(ln) for ln in lines)
    # the text area on the font-pixel grid: every line 16 pixels high, aligned inside the widest line's width
    area = np.zeros((16 * len(lines), 8 * cols), bool)
    for i, ln in enumerate(lines):
        free = 8 * (cols - len(ln))
        x = 0 if st["halign"] == LEFT else free // 2 if st["halign"] == CENTRE else free
        for k, ch in enumerate(ln):
            area[16 * i:16 * i + 16, x + 8 * k:x + 8 * k + 8] = glyph(ch)
    area = np.kron(area.astype(np.uint8), np.ones((s, s), np.uint8)).astype(bool)  # every font pixel s x s samples
    bw, bh = area.shape[1] + 2 * s, area.shape[0] + 2 * s  # the cells' rectangle grown by s on each side
    bx = st["xpad"] if st["halign"] == LEFT else (w - bw) // 2 if st["halign"] == CENTRE else w - st["xpad"] - bw
    by = st["ypad"] if st["valign"] == TOP else (h - bh) // 2 if st["valign"] == 1 else h - st["ypad"] - bh
    bx, by = max(bx, 0) & ~1, max(by, 0) & ~1
    if bx >= w or by >= h:
        return None
    # on a canvas large enough for the whole box, then clipped to the visible size
    ch_, cw_ = max(h, by + bh), max(w, bx + bw)
    T = np.zeros((ch_, cw_), bool)
    T[by + s:by + s + area.shape[0], bx + s:bx + s + area.shape[1]] = area
    B = np.zeros_like(T)
    B[by:by + bh, bx:bx + bw] = True
    # outline: within s samples of a text sample in the 8-neighbourhood sense (Chebyshev distance <= s), not text itself.  T keeps a border of
    # s samples inside B, so the shifts below never wrap a set sample around
    # (the square neighbourhood is taken one axis after the other: the union over |dx| <= s of the union over |dy| <= s is the union over both)
    rows = np.zeros_like(T)
    for dy in range(-s, s + 1):
        rows |= np.roll(T, dy, 0)
    near = np.zeros_like(T)
    for dx in range(-s, s + 1):
        near |= np.roll(rows, dx, 1)
    O = near & ~T
    assert not (O & ~B).any()
    return T[:h, :w], O[:h, :w], B[:h, :w]


def draw(y, uv, text, **style):
    """visible-size planes y (h, w), uv (h / 2, w) -> drawn copies"""
    y, uv = np.array(y, np.uint8), np.array(uv, np.uint8)
    h, w = y.shape
    m = masks(text, w, h, **style)
    if m is None:
        return y, uv
    T, O, B = m
    shaded = dict(DEFAULT, **style)["shaded_background"]
    if shaded:
        bg = B & ~T & ~O
        y[bg] = (y[bg].astype(np.int32) + 16 + 1) >> 1
    y[O] = 16
    y[T] = 235
    ink = T | O
    site = lambda mask: mask[0::2, 0::2] | mask[0::2, 1::2] | mask[1::2, 0::2] | mask[1::2, 1::2]  # any of the site's four luma samples
    si, sb = site(ink), site(B)
    c = uv.reshape(h // 2, w // 2, 2)
    if shaded:
        k = sb & ~si
        c[k] = (c[k].astype(np.int32) + 128 + 1) >> 1
    c[si] = 128
    return y, c.reshape(h // 2, w)


def draw_coded(y, uv, text, **style):
    """... and padded to the coded size by edge replication: what the encoder's source surfaces hold"""
    from tests.util import pad_planes
    return pad_planes(*draw(y, uv, text, **style))
