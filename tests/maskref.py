"""The privacy masks' rule (include/mi355enc.h states it word for word) in numpy, on planes of the visible size: y (h, w) and uv
(h / 2, w) interleaved, both uint8.  A region is a tuple (x, y, w, h, mode, param[, shape[, colour]]): mode 1 fill, 2 pixelate, 3 blur; shape 0 rectangle,
1 ellipse; colour 0xRRGGBB.  Written from the rule's text, not from mask_host.c: the tests hold the two, and the kernels, to ==.  Also the stand-alone
sanitizer driver's pictures, configurations and checksum (csrc/san_mask_driver.c) from the same seed."""
import numpy as np

from tests import autolevelref

FILL, PIXELATE, BLUR = 1, 2, 3
BT601_LIMITED = (16829, 33039, 6416, -9714, -19070, 28784, 28784, -24103, -4681, 16)  # mi355enc_csc_coefficients(6, 0)


def with_margins(y, uv, W, H):
    return autolevelref.with_margins(np.asarray(y), np.asarray(uv), W, H)


def region(r):
    r = tuple(int(v) for v in r)
    return r + (0,) * (8 - len(r))


def colour(rgb, coef):
    """rule 4: 0xRRGGBB -> (Y, Cb, Cr)"""
    c = [int(v) for v in coef]
    r, g, b = (rgb >> 16) & 255, (rgb >> 8) & 255, rgb & 255
    clip = lambda v: max(0, min(255, v))
    return (clip((c[0] * r + c[1] * g + c[2] * b + (c[9] << 16) + 32768) >> 16), clip((c[3] * r + c[4] * g + c[5] * b + (128 << 16) + 32768) >> 16),
            clip((c[6] * r + c[7] * g + c[8] * b + (128 << 16) + 32768) >> 16))


def even_rect(r, w, h):
    """rule 1: (x0, y0, x1, y1) of the even rectangle and (cx0, cy0, cx1, cy1) of its intersection with the picture"""
    x, y, rw, rh = r[:4]
    x0, y0, x1, y1 = x & ~1, y & ~1, (x + rw + 1) & ~1, (y + rh + 1) & ~1
    return (x0, y0, x1, y1), (max(x0, 0), max(y0, 0), min(x1, w), min(y1, h))


def ellipse_inside(W2, H2, qx, qy):
    """rule 2's inequality in Python integers"""
    dx, dy = 2 * (2 * qx + 1) - W2, 2 * (2 * qy + 1) - H2
    return dx * dx * H2 * H2 + dy * dy * W2 * W2 <= W2 * W2 * H2 * H2


def membership(r, w, h):
    """rule 2: bool (h / 2, w / 2), one per 2 x 2 luma quad"""
    (x0, y0, x1, y1), (cx0, cy0, cx1, cy1) = even_rect(r, w, h)
    m = np.zeros((h // 2, w // 2), bool)
    if cx0 >= cx1 or cy0 >= cy1:
        return m
    if not r[6]:
        m[cy0 // 2:cy1 // 2, cx0 // 2:cx1 // 2] = True
        return m
    W2, H2 = x1 - x0, y1 - y0
    qx = np.arange(cx0, cx1, 2, dtype=object) - x0  # (Python integers: no width to overflow)
    qy = np.arange(cy0, cy1, 2, dtype=object) - y0
    dx2, dy2 = (2 * (qx + 1) - W2) ** 2 * (H2 * H2), (2 * (qy + 1) - H2) ** 2 * (W2 * W2)
    m[cy0 // 2:cy1 // 2, cx0 // 2:cx1 // 2] = (dy2[:, None] + dx2[None, :] <= W2 * W2 * H2 * H2).astype(bool)
    return m


def box(p, r, axis):
    """one pass of rule 6 along `axis` of p (rows, n) or (rows, n, 2): positions clamped to the plane, (sum + r) // (2r + 1)"""
    pad = [(0, 0)] * p.ndim
    pad[axis] = (r + 1, r)
    c = np.cumsum(np.pad(p.astype(np.int64), pad, mode="edge"), axis=axis)
    n = p.shape[axis]
    hi = np.take(c, np.arange(2 * r + 1, 2 * r + 1 + n), axis=axis)
    lo = np.take(c, np.arange(0, n), axis=axis)
    return ((hi - lo + r) // (2 * r + 1)).astype(np.uint8)


def blur(y, c, r):
    """rule 6 on a clipped rectangle's luma (ch, cw) and chroma (ch / 2, cw / 2, 2)"""
    rc = (r + 1) >> 1
    for _ in range(2):
        y, c = box(box(y, r, 1), r, 0), box(box(c, rc, 1), rc, 0)
    return y, c


def pixelate(y, c, cell, ox, oy):
    """rule 5 on a clipped rectangle's luma and chroma; (ox, oy): where the clipped rectangle starts inside the even one (the grid's origin is the even one's)"""
    ch, cw = y.shape
    oy_, oc_ = y.copy(), c.copy()
    for gy in range(-oy, ch, cell):
        for gx in range(-ox, cw, cell):
            ax, ay, bx, by = max(gx, 0), max(gy, 0), min(gx + cell, cw), min(gy + cell, ch)
            if ax >= bx or ay >= by:
                continue
            s = y[ay:by, ax:bx].astype(np.int64)
            oy_[ay:by, ax:bx] = (int(s.sum()) + s.size // 2) // s.size
            for k in range(2):
                s = c[ay // 2:by // 2, ax // 2:bx // 2, k].astype(np.int64)
                oc_[ay // 2:by // 2, ax // 2:bx // 2, k] = (int(s.sum()) + s.size // 2) // s.size
    return oy_, oc_


def apply(y, uv, regions, coef=BT601_LIMITED):
    """rules 1 .. 6 -> new (y, uv)"""
    y, uv = np.asarray(y, np.uint8), np.asarray(uv, np.uint8)
    h, w = y.shape
    src_y, src_c = y, uv.reshape(h // 2, w // 2, 2)
    out_y, out_c = src_y.copy(), src_c.copy()
    taken = np.zeros((h // 2, w // 2), bool)
    for r in map(region, regions):
        (x0, y0, x1, y1), (cx0, cy0, cx1, cy1) = even_rect(r, w, h)
        if cx0 >= cx1 or cy0 >= cy1:
            continue
        own = membership(r, w, h) & ~taken  # rule 3: the lowest index wins
        taken |= own
        ry, rc = src_y[cy0:cy1, cx0:cx1], src_c[cy0 // 2:cy1 // 2, cx0 // 2:cx1 // 2]
        if r[4] == FILL:
            f = colour(r[7], coef)
            ry, rc = np.full_like(ry, f[0]), np.broadcast_to(np.array(f[1:], np.uint8), rc.shape)
        elif r[4] == PIXELATE:
            ry, rc = pixelate(ry, rc, r[5], cx0 - x0, cy0 - y0)
        else:
            ry, rc = blur(ry, rc, r[5])
        q = own[cy0 // 2:cy1 // 2, cx0 // 2:cx1 // 2]
        out_c[cy0 // 2:cy1 // 2, cx0 // 2:cx1 // 2][q] = rc[q]
        out_y[cy0:cy1, cx0:cx1][np.repeat(np.repeat(q, 2, 0), 2, 1)] = ry[np.repeat(np.repeat(q, 2, 0), 2, 1)]
    return out_y, out_c.reshape(h // 2, w)


def coded(y, uv, regions, W, H, coef=BT601_LIMITED):
    """what the launches leave of a coded-size picture whose margins are replicas: rule 7"""
    vy, vuv = apply(y, uv, regions, coef)
    return with_margins(vy, vuv, W, H)


def to_text(regions):
    """the element's string form"""
    return ";".join(",".join(str(v) for v in region(r)[:7]) for r in regions)


# ---- the sanitizer driver's side (csrc/san_mask_driver.c): the same generator, pictures, configurations and checksum
class Rng:
    def __init__(self):
        self.s = 0x9E3779B9

    def next(self):
        s = self.s
        s ^= (s << 13) & 0xFFFFFFFF
        s ^= s >> 17
        s ^= (s << 5) & 0xFFFFFFFF
        self.s = s
        return s

    def between(self, lo, hi):
        return lo + self.next() % (hi - lo + 1)


def driver_picture(seed, w, h):
    """byte i of a picture's w h 3 / 2 bytes: a hash of i and the seed, in 32-bit arithmetic"""
    i = np.arange(w * h * 3 // 2, dtype=np.uint64)
    v = (i * 2654435761 + seed) & 0xFFFFFFFF
    v ^= v >> 15
    v = (v * 2246822519) & 0xFFFFFFFF
    v ^= v >> 13
    b = (v & 255).astype(np.uint8)
    return b[:w * h].reshape(h, w), b[w * h:].reshape(h // 2, w)


def driver_digest(y, uv):
    b = np.concatenate([y.reshape(-1), uv.reshape(-1)]).astype(np.uint64)
    k = (np.arange(b.size, dtype=np.uint64) * 2654435761 + 12345) & 0xFFFFFFFF
    return int((b * k).sum(dtype=np.uint64) & 0xFFFFFFFF)


DRIVER_BASE = (3, 5, 9, 7, BLUR, 2, 0, 0x204060)
DRIVER_EDGES = [  # (field, values accepted at its edges) -- mode and param together
    (0, (-16384, 16384)), (1, (-16384, 16384)), (2, (1, 16384)), (3, (1, 16384)), (6, (0, 1)), (7, (0, 0xFFFFFF))]
DRIVER_MODES = [(FILL, 0), (PIXELATE, 4), (PIXELATE, 64), (BLUR, 1), (BLUR, 32)]
DRIVER_BEYOND = [(-40, 4, 60, 12), (-100, 4, 100, 12), (-100, 4, 99, 12), (30, 4, 100, 12), (42, 4, 10, 12), (41, 4, 1, 12), (4, -30, 12, 50), (4, -50, 12, 50),
                 (4, 20, 12, 50), (4, 26, 12, 50), (-16384, -16384, 16384, 16384), (-16383, -16383, 16384, 16384), (-16384 + 20, -16384 + 12, 16384, 16384)]
DRIVER_SIZES = [(16, 16), (42, 26), (70, 50), (18, 34)]


def driver_cases():
    """every (w, h, seed, regions) the driver applies, in its order"""
    g = Rng()
    out = []

    def one(w, h, regions):
        out.append((w, h, g.next(), [region(r) for r in regions]))

    for f, vals in DRIVER_EDGES:
        for v in vals:
            r = list(DRIVER_BASE)
            r[f] = v
            one(16, 16, [r])
    for mode, param in DRIVER_MODES:
        r = list(DRIVER_BASE)
        r[4], r[5] = mode, param
        one(16, 16, [r])
        one(70, 50, [(1, 1, 67, 47, mode, param, 1, 0x808080)])
    one(16, 16, [DRIVER_BASE] * 8)
    one(16, 16, [])
    for i, (x, y, w, h) in enumerate(DRIVER_BEYOND):
        for shape in (0, 1):
            one(42, 26, [(x, y, w, h, 1 + i % 3, (0, 6, 5)[i % 3], shape, 0x10F0A0)])
    for w, h in ((16, 16), (8192, 16)):
        one(w, h, [(0, 0, w, h, BLUR, 32, 0, 0)])
        one(w, h, [(-5, -3, w + 9, h + 7, PIXELATE, 64, 1, 0)])
        one(w, h, [(w - 3, h - 3, 3, 3, FILL, 0, 0, 0xFF0000), (1, 1, w - 2, h - 2, BLUR, 7, 1, 0), (0, 0, w, h, PIXELATE, 6, 0, 0)])
    for i in range(200):
        w, h = DRIVER_SIZES[i % 4]
        regs = []
        for _ in range(g.between(0, 8)):
            x, y, rw, rh = g.between(-20, w + 10), g.between(-20, h + 10), g.between(1, w + 30), g.between(1, h + 30)
            mode = g.between(1, 3)
            param = 0 if mode == FILL else 2 * g.between(2, 32) if mode == PIXELATE else g.between(1, 32)
            regs.append((x, y, rw, rh, mode, param, g.between(0, 1), g.next() & 0xFFFFFF))
        one(w, h, regs)
    return out


def driver_checksum():
    """(FNV-1a over every picture's digest, the count of pictures)"""
    fnv = 2166136261
    cases = driver_cases()
    for w, h, seed, regs in cases:
        d = driver_digest(*apply(*driver_picture(seed, w, h), regs))
        for k in range(4):
            fnv = ((fnv ^ ((d >> (8 * k)) & 255)) * 16777619) & 0xFFFFFFFF
    return fnv, len(cases)
