"""numpy restatement of DESIGN.md section 20, written from the rule's text: the colour step (YUV of one range and matrix -> YUV of another) and the
10-bit / grey input formats.

The colour step, pointwise on NV12 (a luma sample uses the chroma pair of its own 2 x 2 block).  r(x) = floor(x + 0.5) in IEEE double; (Kr, Kb) per matrix
code, Kg = 1 - Kr - Kb; primes denote the output; Ys = 219 | 255, Cs = 224 | 255, oy = 16 | 0 (limited | full range):
  lb = 2 (1 - Kb) (Kb' - Kg' Kb / Kg),  lr = 2 (1 - Kr) (Kr' - Kg' Kr / Kg)
  cyy = r(Ys' / Ys 2^16)   cyb = r(lb Ys' / Cs 2^16)   cyr = r(lr Ys' / Cs 2^16)
  cbb = r((2 (1 - Kb) - lb) / (2 (1 - Kb')) Cs' / Cs 2^16)   cbr = r(-lr / (2 (1 - Kb')) Cs' / Cs 2^16)
  crb = r(-lb / (2 (1 - Kr')) Cs' / Cs 2^16)                 crr = r((2 (1 - Kr) - lr) / (2 (1 - Kr')) Cs' / Cs 2^16)
  Y'  = clip255((cyy (Y - oy) + cyb (Cb - 128) + cyr (Cr - 128) + (oy' << 16) + 2^15) >> 16)
  Cb' = clip255((cbb (Cb - 128) + cbr (Cr - 128) + (128 << 16) + 2^15) >> 16),  Cr' likewise with crb, crr
With a geometry the border is not converted: a coded sample is picture iff its clamped visible source (min(x, vis_w - 1), min(y, vis_h - 1)) lies in the
destination rectangle mapped through the orientation.

10 -> 8 bits: y8 = min(255, (v10 + 2) >> 2), a 4:2:0 chroma sample likewise, a 4:2:2 one from the sum S of its two rows, min(255, (S + 4) >> 3).
P010: 16-bit words, v10 = word >> 6.  I420_10: v10 = word & 1023.  v210: six pixels in four 32-bit words of three 10-bit fields (bits 0-9, 10-19, 20-29):
Cb0 Y0 Cr0 | Y1 Cb1 Y2 | Cr1 Y3 Cb2 | Y4 Cr2 Y5; a row reads ceil(w / 6) 16 bytes.  GRAY8: luma copied, every chroma byte 128.
Planes are handled as rows of bytes (uint8, little-endian words), the way the library is handed them.
"""
import numpy as np

from oracle.csc import _pad

FMT_P010, FMT_I420_10, FMT_V210, FMT_GRAY8 = 14, 15, 16, 17
DEEP_FMTS = [FMT_P010, FMT_I420_10, FMT_V210, FMT_GRAY8]
NAMES = {FMT_P010: "P010", FMT_I420_10: "I420_10", FMT_V210: "v210", FMT_GRAY8: "GRAY8"}
KR_KB = {1: (0.2126, 0.0722), 5: (0.299, 0.114), 6: (0.299, 0.114), 9: (0.2627, 0.0593)}
TRANSPOSING = (1, 3, 6, 7)


def _r(x):
    return int(np.floor(x + 0.5))


def _terms(in_m, in_full, out_m, out_full):
    kr, kb = KR_KB[in_m]
    kr2, kb2 = KR_KB[out_m]
    kg, kg2 = 1.0 - kr - kb, 1.0 - kr2 - kb2
    ys, cs = (255.0, 255.0) if in_full else (219.0, 224.0)
    ys2, cs2 = (255.0, 255.0) if out_full else (219.0, 224.0)
    lb = 2.0 * (1.0 - kb) * (kb2 - kg2 * kb / kg)
    lr = 2.0 * (1.0 - kr) * (kr2 - kg2 * kr / kg)
    return [ys2 / ys,
            lb * ys2 / cs,
            lr * ys2 / cs,
            (2.0 * (1.0 - kb) - lb) / (2.0 * (1.0 - kb2)) * cs2 / cs,
            -lr / (2.0 * (1.0 - kb2)) * cs2 / cs,
            -lb / (2.0 * (1.0 - kr2)) * cs2 / cs,
            (2.0 * (1.0 - kr) - lr) / (2.0 * (1.0 - kr2)) * cs2 / cs]


def coefficients(in_m, in_full, out_m, out_full):
    """-> [cyy, cyb, cyr, cbb, cbr, crb, crr, oy, oy']"""
    return [_r(t * 65536.0) for t in _terms(in_m, in_full, out_m, out_full)] + [0 if in_full else 16, 0 if out_full else 16]


def exact(in_m, in_full, out_m, out_full, y, cb, cr):
    """the unrounded double-precision Y', Cb', Cr' of samples y, cb, cr (arrays)"""
    t = _terms(in_m, in_full, out_m, out_full)
    oy, oy2 = (0.0 if in_full else 16.0), (0.0 if out_full else 16.0)
    y, cb, cr = (np.asarray(v, np.float64) for v in (y, cb, cr))
    return (oy2 + t[0] * (y - oy) + t[1] * (cb - 128.0) + t[2] * (cr - 128.0),
            128.0 + t[3] * (cb - 128.0) + t[4] * (cr - 128.0),
            128.0 + t[5] * (cb - 128.0) + t[6] * (cr - 128.0))


def unclipped(coef, y, cb, cr):
    """the integer results before the clip (int64 arrays)"""
    cyy, cyb, cyr, cbb, cbr, crb, crr, oy, oy2 = (int(c) for c in coef)
    y, cb, cr = (np.asarray(v).astype(np.int64) for v in (y, cb, cr))
    return ((cyy * (y - oy) + cyb * (cb - 128) + cyr * (cr - 128) + (oy2 << 16) + (1 << 15)) >> 16,
            (cbb * (cb - 128) + cbr * (cr - 128) + (128 << 16) + (1 << 15)) >> 16,
            (crb * (cb - 128) + crr * (cr - 128) + (128 << 16) + (1 << 15)) >> 16)


def convert(y, uv, coef, mask=None):
    """NV12 planes (y (H, W), uv (H / 2, W) interleaved) -> the converted copies; mask (H, W) bool: the luma samples that are picture (constant over every 2 x 2
    block), everything else keeps its bytes"""
    y, uv = np.asarray(y, np.uint8), np.asarray(uv, np.uint8)
    cb, cr = uv[:, 0::2], uv[:, 1::2]
    up = lambda c: np.repeat(np.repeat(c, 2, 0), 2, 1)
    ny, _, _ = unclipped(coef, y, up(cb), up(cr))
    _, nb, nr = unclipped(coef, 0, cb, cr)
    oy = np.clip(ny, 0, 255).astype(np.uint8)
    ouv = np.empty_like(uv)
    ouv[:, 0::2], ouv[:, 1::2] = np.clip(nb, 0, 255), np.clip(nr, 0, 255)
    if mask is not None:
        mask = np.asarray(mask, bool)
        assert np.array_equal(mask, up(mask[0::2, 0::2]))
        oy = np.where(mask, oy, y)
        ouv = np.where(np.repeat(mask[0::2, 0::2], 2, 1), ouv, uv)
    return oy, ouv


def orient_source(method, out_w, out_h, x, y):
    """the pre-orientation sample the oriented picture's (x, y) shows (GstVideoOrientationMethod; arrays welcome)"""
    tr = method in TRANSPOSING
    in_w, in_h = (out_h, out_w) if tr else (out_w, out_h)
    u, v = (y, x) if tr else (x, y)
    sx = in_w - 1 - u if method in (2, 3, 4, 7) else u
    sy = in_h - 1 - v if method in (1, 2, 5, 7) else v
    return sx, sy


def picture_mask(vis_w, vis_h, dst=None, method=0):
    """(H, W) bool over the coded surfaces: True where a sample is picture.  dst (x, y, w, h): the geometry's destination rectangle inside the pre-orientation
    target (None: no geometry, everything is picture); method: the orientation"""
    W, H = (vis_w + 15) // 16 * 16, (vis_h + 15) // 16 * 16
    if dst is None:
        return np.ones((H, W), bool)
    xs, ys = np.meshgrid(np.minimum(np.arange(W), vis_w - 1), np.minimum(np.arange(H), vis_h - 1))
    sx, sy = orient_source(method, vis_w, vis_h, xs, ys)
    dx, dy, dw, dh = dst
    return (sx >= dx) & (sx < dx + dw) & (sy >= dy) & (sy < dy + dh)


# ---- the formats
def _words(plane, rows, nbytes, dtype):
    """the first nbytes of each of the first `rows` rows of a byte plane, as little-endian words"""
    p = np.ascontiguousarray(np.asarray(plane, np.uint8)[:rows, :nbytes])
    return p.view(dtype).astype(np.int64)


def unpack_p010(planes, w, h):
    """-> 10-bit (Y (h, w), Cb, Cr (h / 2, w / 2))"""
    y = _words(planes[0], h, 2 * w, "<u2") >> 6
    c = _words(planes[1], h // 2, 2 * w, "<u2") >> 6
    return y, c[:, 0::2], c[:, 1::2]


def unpack_i420_10(planes, w, h):
    return (_words(planes[0], h, 2 * w, "<u2") & 1023, _words(planes[1], h // 2, w, "<u2") & 1023, _words(planes[2], h // 2, w, "<u2") & 1023)


# (word, shift) of the six luma and the six chroma samples (Cb0 Cr0 Cb1 Cr1 Cb2 Cr2) of a group
V210_Y = ((0, 10), (1, 0), (1, 20), (2, 10), (3, 0), (3, 20))
V210_C = ((0, 0), (0, 20), (1, 10), (2, 0), (2, 20), (3, 10))


def v210_row_bytes(w):
    return (w + 5) // 6 * 16


def unpack_v210(plane, w, h):
    """-> 10-bit (Y (h, w), Cb, Cr (h, w / 2)): 4:2:2"""
    g = (w + 5) // 6
    words = _words(plane, h, 16 * g, "<u4").reshape(h, g, 4)
    y = np.stack([(words[:, :, wi] >> sh) & 1023 for wi, sh in V210_Y], axis=2).reshape(h, 6 * g)
    c = np.stack([(words[:, :, wi] >> sh) & 1023 for wi, sh in V210_C], axis=2).reshape(h, 3 * g, 2)
    return y[:, :w], c[:, :w // 2, 0], c[:, :w // 2, 1]


def pack_v210(y, cb, cr, rng=None):
    """10-bit Y (h, w), Cb, Cr (h, w / 2) -> a byte plane (h, ceil(w / 6) 16); samples past the width are 0; rng: bits 30 - 31 of every word at random"""
    y, cb, cr = (np.asarray(v).astype(np.int64) for v in (y, cb, cr))
    h, w = y.shape
    g = (w + 5) // 6
    yy = np.zeros((h, 6 * g), np.int64)
    yy[:, :w] = y
    cc = np.zeros((h, 3 * g, 2), np.int64)
    cc[:, :w // 2, 0], cc[:, :w // 2, 1] = cb, cr
    yy, cc = yy.reshape(h, g, 6), cc.reshape(h, g, 6)
    words = np.zeros((h, g, 4), np.int64)
    for k, (wi, sh) in enumerate(V210_Y):
        words[:, :, wi] |= yy[:, :, k] << sh
    for k, (wi, sh) in enumerate(V210_C):
        words[:, :, wi] |= cc[:, :, k] << sh
    if rng is not None:
        words |= rng.integers(0, 4, words.shape, dtype=np.int64) << 30
    return np.ascontiguousarray(words.astype("<u4")).view(np.uint8).reshape(h, 16 * g)


def down8(v10):
    return np.minimum(255, (np.asarray(v10).astype(np.int64) + 2) >> 2)


def down8_rows(a, b):
    """a 4:2:2 chroma sample from its two rows"""
    return np.minimum(255, (np.asarray(a).astype(np.int64) + np.asarray(b).astype(np.int64) + 4) >> 3)


def _interleave(u, v):
    uv = np.empty((u.shape[0], 2 * u.shape[1]), np.uint8)
    uv[:, 0::2], uv[:, 1::2] = u, v
    return uv


def to_nv12(fmt, planes, w, h):
    """-> the coded-size (multiples of 16) NV12 surfaces (Y, UV); the margin repeats the last visible row / column / chroma pair"""
    W, H = (w + 15) // 16 * 16, (h + 15) // 16 * 16
    if fmt == FMT_P010:
        y, u, v = (down8(c) for c in unpack_p010(planes, w, h))
    elif fmt == FMT_I420_10:
        y, u, v = (down8(c) for c in unpack_i420_10(planes, w, h))
    elif fmt == FMT_V210:
        y10, u10, v10 = unpack_v210(planes[0], w, h)
        y, u, v = down8(y10), down8_rows(u10[0::2], u10[1::2]), down8_rows(v10[0::2], v10[1::2])
    elif fmt == FMT_GRAY8:
        y = np.asarray(planes[0], np.uint8)[:h, :w]
        u = v = np.full((h // 2, w // 2), 128, np.uint8)
    else:
        raise ValueError(fmt)
    return _pad(np.ascontiguousarray(y.astype(np.uint8)), H, W, False), _pad(_interleave(u.astype(np.uint8), v.astype(np.uint8)), H // 2, W, True)


def random_planes(fmt, w, h, rng, pad=0, offset=0):
    """random byte planes of a w x h picture in `fmt`, the bits the format ignores (P010's low six, I420_10's high six, v210's bits 30 - 31) set at random;
    pad: extra bytes per row, offset: where the first sample lies in its buffer"""
    def mk(rows, nbytes):
        buf = rng.integers(0, 256, rows * (nbytes + pad) + offset, dtype=np.uint8)
        return np.lib.stride_tricks.as_strided(buf[offset:], (rows, nbytes), (nbytes + pad, 1))
    if fmt == FMT_P010:
        return [mk(h, 2 * w), mk(h // 2, 2 * w)]
    if fmt == FMT_I420_10:
        return [mk(h, 2 * w), mk(h // 2, w), mk(h // 2, w)]
    if fmt == FMT_V210:
        return [mk(h, v210_row_bytes(w))]
    if fmt == FMT_GRAY8:
        return [mk(h, w)]
    raise ValueError(fmt)
