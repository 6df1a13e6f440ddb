"""numpy restatement of the conversion rule for the input formats of k_csc.hip, written from the rule's text:

- visible width and height even; the coded-size margin repeats the last visible row / column / chroma pair;
- YV12, NV21: I420 / NV12 with the chroma roles exchanged.  Y42B: luma copied, chroma the rounded mean of its two rows, (a + b + 1) >> 1;
- 4:4:4 -> 4:2:0 (Y444 chroma, and R, G, B before the matrix): weights [1 2 1] over columns 2i - 1, 2i, 2i + 1 (clamped to the picture) times
  [1 1] over rows 2j, 2j + 1, sum 8; Y444: c = (S + 4) >> 3;
- RGB 0 .. 255 -> Y'CbCr with integer coefficients in 2^-16 units derived in double from (Kr, Kb) of the matrix code and the range:
  Y = clip((yr R + yg G + yb B + (off << 16) + 2^15) >> 16), Cb = clip((br S_R + bg S_G + bb S_B + (128 << 19) + 2^18) >> 19), Cr likewise.
"""
import numpy as np

from oracle.csc import _pad

FMT_NV12, FMT_I420, FMT_YUY2, FMT_UYVY, FMT_Y42B, FMT_Y444, FMT_YV12, FMT_NV21, FMT_BGRX, FMT_RGBX, FMT_XRGB, FMT_XBGR, FMT_BGR, FMT_RGB = range(14)
NEW_FMTS = list(range(FMT_Y42B, FMT_RGB + 1))
RGB_FMTS = list(range(FMT_BGRX, FMT_RGB + 1))
NAMES = {FMT_Y42B: "Y42B", FMT_Y444: "Y444", FMT_YV12: "YV12", FMT_NV21: "NV21", FMT_BGRX: "BGRx", FMT_RGBX: "RGBx", FMT_XRGB: "xRGB", FMT_XBGR: "xBGR",
         FMT_BGR: "BGR", FMT_RGB: "RGB"}
# bytes per pixel and the byte of R, G, B inside a pixel
RGB_LAYOUT = {FMT_BGRX: (4, 2, 1, 0), FMT_RGBX: (4, 0, 1, 2), FMT_XRGB: (4, 1, 2, 3), FMT_XBGR: (4, 3, 2, 1), FMT_BGR: (3, 2, 1, 0), FMT_RGB: (3, 0, 1, 2)}
KR_KB = {1: (0.2126, 0.0722), 5: (0.299, 0.114), 6: (0.299, 0.114), 9: (0.2627, 0.0593)}
MATRIX_RANGE_PAIRS = [(m, fr) for m in (1, 5, 6, 9) for fr in (0, 1)]


def resolve_matrix(matrix, width, height):
    """code 2 (unspecified): BT.709 for a coded picture wider than 1024 or higher than 576, else BT.601"""
    if matrix == 2:
        return 1 if (width > 1024 or height > 576) else 6
    return matrix


def _r(x):
    return int(np.floor(x + 0.5))


def coefficients(matrix, full_range):
    """-> [yr, yg, yb, br, bg, bb, rr, rg, rb, off]"""
    kr, kb = KR_KB[matrix]
    sy, sc, off = (1.0, 1.0, 0) if full_range else (219.0 / 255.0, 224.0 / 255.0, 16)
    yr, yb = _r(kr * sy * 65536.0), _r(kb * sy * 65536.0)
    yg = _r(sy * 65536.0) - yr - yb
    bb = _r(0.5 * sc * 65536.0)
    br = -_r(kr / (2.0 * (1.0 - kb)) * sc * 65536.0)
    bg = -bb - br
    rr = _r(0.5 * sc * 65536.0)
    rb = -_r(kb / (2.0 * (1.0 - kr)) * sc * 65536.0)
    rg = -rr - rb
    return [yr, yg, yb, br, bg, bb, rr, rg, rb, off]


def exact(matrix, full_range, r, g, b):
    """the unrounded double-precision Y', Cb, Cr of colours r, g, b (arrays)"""
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    sy, sc, off = (1.0, 1.0, 0.0) if full_range else (219.0 / 255.0, 224.0 / 255.0, 16.0)
    r, g, b = (np.asarray(v, np.float64) for v in (r, g, b))
    y = kr * r + kg * g + kb * b
    return off + sy * y, 128.0 + sc * (b - y) / (2.0 * (1.0 - kb)), 128.0 + sc * (r - y) / (2.0 * (1.0 - kr))


def tap8(plane):
    """the eight-weight sums of a (h, w) plane at the 4:2:0 sites: (h / 2, w / 2) int64"""
    p = np.asarray(plane).astype(np.int64)
    h, w = p.shape
    cols = np.arange(0, w, 2)
    hsum = p[:, np.clip(cols - 1, 0, w - 1)] + 2 * p[:, cols] + p[:, np.clip(cols + 1, 0, w - 1)]
    return hsum[0::2] + hsum[1::2]


def rgb_pixel(coef, r, g, b):
    """one colour over a whole 2 x 2 site (the sums are 8 times the colour) -> (Y, Cb, Cr)"""
    yr, yg, yb, br, bg, bb, rr, rg, rb, off = coef
    r, g, b = (np.asarray(v).astype(np.int64) for v in (r, g, b))
    y = np.clip((yr * r + yg * g + yb * b + (off << 16) + (1 << 15)) >> 16, 0, 255)
    cb = np.clip((br * 8 * r + bg * 8 * g + bb * 8 * b + (128 << 19) + (1 << 18)) >> 19, 0, 255)
    cr = np.clip((rr * 8 * r + rg * 8 * g + rb * 8 * b + (128 << 19) + (1 << 18)) >> 19, 0, 255)
    return y, cb, cr


def rgb_planes(fmt, plane, width, height):
    bpp, ro, go, bo = RGB_LAYOUT[fmt]
    p = np.asarray(plane, np.uint8)[:height, :bpp * width]
    return p[:, ro::bpp], p[:, go::bpp], p[:, bo::bpp]


def rgb_sums(fmt, plane, width, height):
    """(R, G, B, S_R, S_G, S_B) of a packed RGB picture: the components per pixel and their eight-weight sums per 4:2:0 site"""
    r, g, b = (c.astype(np.int64) for c in rgb_planes(fmt, plane, width, height))
    return r, g, b, tap8(r), tap8(g), tap8(b)


def rgb_convert(sums, coef):
    """-> visible-size Y, Cb, Cr planes from rgb_sums() and coefficients()"""
    r, g, b, sr, sg, sb = sums
    yr, yg, yb, br, bg, bb, rr, rg, rb, off = coef
    y = np.clip((yr * r + yg * g + yb * b + (off << 16) + (1 << 15)) >> 16, 0, 255).astype(np.uint8)
    u = np.clip((br * sr + bg * sg + bb * sb + (128 << 19) + (1 << 18)) >> 19, 0, 255).astype(np.uint8)
    v = np.clip((rr * sr + rg * sg + rb * sb + (128 << 19) + (1 << 18)) >> 19, 0, 255).astype(np.uint8)
    return y, u, v


def pad_nv12(y, u, v):
    """visible-size planes -> the coded-size NV12 surfaces"""
    h, w = y.shape
    W, H = (w + 15) // 16 * 16, (h + 15) // 16 * 16
    return _pad(np.ascontiguousarray(y), H, W, False), _pad(_interleave(u, v), H // 2, W, True)


def _interleave(u, v):
    uv = np.empty((u.shape[0], 2 * u.shape[1]), np.uint8)
    uv[:, 0::2], uv[:, 1::2] = u, v
    return uv


def to_nv12(fmt, planes, width, height, matrix=2, full_range=0, coded=None):
    """-> the coded-size (multiples of 16) NV12 surfaces (Y, UV).  matrix / full_range: the handle's colorimetry (RGB formats); coded: the
    (width, height) the matrix code 2 is resolved with, when it is not the picture's own size (scaled input)."""
    W, H = (width + 15) // 16 * 16, (height + 15) // 16 * 16
    hw, hh = width // 2, height // 2
    if fmt in (FMT_YV12, FMT_I420):
        y = np.asarray(planes[0], np.uint8)[:height, :width]
        u, v = (np.asarray(p, np.uint8)[:hh, :hw] for p in (planes[1:3] if fmt == FMT_I420 else (planes[2], planes[1])))
    elif fmt == FMT_NV21:
        y, vu = np.asarray(planes[0], np.uint8)[:height, :width], np.asarray(planes[1], np.uint8)[:hh, :width]
        u, v = vu[:, 1::2], vu[:, 0::2]
    elif fmt == FMT_Y42B:
        y = np.asarray(planes[0], np.uint8)[:height, :width]
        u, v = (((c[0::2] + c[1::2] + 1) >> 1).astype(np.uint8) for c in (np.asarray(p, np.uint8)[:height, :hw].astype(np.uint16) for p in planes[1:3]))
    elif fmt == FMT_Y444:
        y = np.asarray(planes[0], np.uint8)[:height, :width]
        u, v = (((tap8(np.asarray(p, np.uint8)[:height, :width]) + 4) >> 3).astype(np.uint8) for p in planes[1:3])
    elif fmt in RGB_LAYOUT:
        cw, ch = coded if coded is not None else (width, height)
        y, u, v = rgb_convert(rgb_sums(fmt, planes[0], width, height), coefficients(resolve_matrix(matrix, cw, ch), full_range))
    else:
        raise ValueError(fmt)
    return _pad(np.ascontiguousarray(y), H, W, False), _pad(_interleave(u, v), H // 2, W, True)


def random_planes(fmt, w, h, rng, pad=0, offset=0):
    """random planes of a w x h picture in `fmt`; pad: extra bytes per row, offset: where the first sample lies in its buffer"""
    def mk(rows, cols):
        buf = rng.integers(0, 256, rows * (cols + pad) + offset, dtype=np.uint8)
        return np.lib.stride_tricks.as_strided(buf[offset:], (rows, cols), (cols + pad, 1))
    if fmt in (FMT_I420, FMT_YV12):
        return [mk(h, w), mk(h // 2, w // 2), mk(h // 2, w // 2)]
    if fmt == FMT_Y42B:
        return [mk(h, w), mk(h, w // 2), mk(h, w // 2)]
    if fmt == FMT_Y444:
        return [mk(h, w), mk(h, w), mk(h, w)]
    if fmt in (FMT_NV12, FMT_NV21):
        return [mk(h, w), mk(h // 2, w)]
    if fmt in (FMT_YUY2, FMT_UYVY):
        return [mk(h, 2 * w)]
    return [mk(h, RGB_LAYOUT[fmt][0] * w)]
