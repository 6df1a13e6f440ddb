"""The image layers' blending rule in numpy, written from the rule's text on whole planes.  All arithmetic is integer
(int64 here; the rule fits 32 bits).  The rule works on the visible NV12 picture (w x h, both even); the coded-size surfaces follow by edge
replication (tests/util.py pad_planes), "as if the images had been in the picture before padding".

A layer is a dict: pixels (ih, iw, 4) uint8 with straight alpha in byte order fmt, the place x, y of its top-left pixel in visible luma
coordinates (any integer), opacity 0 .. 256.  Layers are blended in list order, each onto the result of the one before."""
import numpy as np

from tests import cscref

FMT_BGRA, FMT_RGBA, FMT_ARGB, FMT_ABGR = cscref.FMT_BGRX, cscref.FMT_RGBX, cscref.FMT_XRGB, cscref.FMT_XBGR
FMTS = (FMT_BGRA, FMT_RGBA, FMT_ARGB, FMT_ABGR)
# the byte of R, G, B, A inside a pixel
LAYOUT = {FMT_BGRA: (2, 1, 0, 3), FMT_RGBA: (0, 1, 2, 3), FMT_ARGB: (1, 2, 3, 0), FMT_ABGR: (3, 2, 1, 0)}
LAYERS, MAX_DIM, PLACE_MAX = 4, 4096, 16384


def coefficients(matrix, full_range, w, h):
    """the ten words the handle converts RGB with: matrix 2 (unspecified) is decided by the coded size"""
    return cscref.coefficients(cscref.resolve_matrix(matrix, w, h), full_range)


def pixel(coef, r, g, b):
    """(Yi, Cbi, Cri) of colours r, g, b (arrays or numbers): every component rounded and clipped on its own, the shifts arithmetic"""
    yr, yg, yb, br, bg, bb, rr, rg, rb, off = (int(c) for c in coef)
    r, g, b = (np.asarray(v).astype(np.int64) for v in (r, g, b))
    yi = np.clip((yr * r + yg * g + yb * b + (off << 16) + (1 << 15)) >> 16, 0, 255)
    cb = np.clip((br * r + bg * g + bb * b + (128 << 16) + (1 << 15)) >> 16, 0, 255)
    cr = np.clip((rr * r + rg * g + rb * b + (128 << 16) + (1 << 15)) >> 16, 0, 255)
    return yi, cb, cr


def rgba(pixels, fmt):
    """pixels in byte order fmt -> (ih, iw, 4) in the order R, G, B, A"""
    p = np.asarray(pixels, np.uint8)
    return p[:, :, list(LAYOUT[fmt])]


def to_fmt(pix_rgba, fmt):
    """RGBA pixels -> byte order fmt"""
    out = np.empty_like(np.asarray(pix_rgba, np.uint8))
    for k, pos in enumerate(LAYOUT[fmt]):
        out[:, :, pos] = pix_rgba[:, :, k]
    return out


def layer(pixels, x=0, y=0, opacity=256, fmt=FMT_RGBA):
    return dict(pixels=np.asarray(pixels, np.uint8), x=int(x), y=int(y), opacity=int(opacity), fmt=fmt)


def _canvas(ly, coef, w, h):
    """the layer on the visible luma grid: (a, Yi, Cbi, Cri) int64 (h, w); a = 0 where the image does not cover a sample"""
    p = rgba(ly["pixels"], ly["fmt"]).astype(np.int64)
    ih, iw = p.shape[:2]
    yi, cb, cr = pixel(coef, p[:, :, 0], p[:, :, 1], p[:, :, 2])
    a = (p[:, :, 3] * ly["opacity"] + 128) >> 8
    out = np.zeros((4, h, w), np.int64)
    x, y = ly["x"], ly["y"]
    x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + iw, w), min(y + ih, h)
    if x0 < x1 and y0 < y1:
        for k, src in enumerate((a, yi, cb, cr)):
            out[k, y0:y1, x0:x1] = src[y0 - y:y1 - y, x0 - x:x1 - x]
    return out


def blend(y, uv, layers, coef):
    """visible-size planes y (h, w), uv (h / 2, w) -> blended copies"""
    y, uv = np.array(y, np.uint8), np.array(uv, np.uint8)
    h, w = y.shape
    assert h % 2 == 0 and w % 2 == 0 and uv.shape == (h // 2, w)
    for ly in layers:
        if ly is None or ly.get("pixels") is None:
            continue
        a, yi, cbi, cri = _canvas(ly, coef, w, h)
        d = y.astype(np.int64)
        y = ((d * (255 - a) + yi * a + 127) // 255).astype(np.uint8)  # (a = 0: d * 255 + 127 over 255 is d)
        quad = lambda m: m[0::2, 0::2] + m[0::2, 1::2] + m[1::2, 0::2] + m[1::2, 1::2]
        sa = quad(a)
        c = uv.reshape(h // 2, w // 2, 2).astype(np.int64)
        cb = (c[:, :, 0] * (1020 - sa) + quad(a * cbi) + 510) // 1020
        cr = (c[:, :, 1] * (1020 - sa) + quad(a * cri) + 510) // 1020
        uv = np.stack([cb, cr], axis=2).astype(np.uint8).reshape(h // 2, w)
    return y, uv


def blend_coded(y, uv, layers, coef):
    """... and padded to the coded size by edge replication: what the encoder's source surfaces hold"""
    from tests.util import pad_planes
    return pad_planes(*blend(y, uv, layers, coef))


def random_image(rng, iw, ih):
    """seeded random RGBA pixels: at least a quarter of the alphas (rounded up) 255 and as many 0 -- a 1 x 1 image has room for one of the two: 255"""
    p = rng.integers(0, 256, (ih, iw, 4), dtype=np.uint8)
    n = iw * ih
    q, idx = -(-n // 4), rng.permutation(n)
    al = p[:, :, 3].reshape(-1)  # (a view: p is contiguous)
    al[idx[q:2 * q]] = 0
    al[idx[:q]] = 255
    return p


def pam(pix_rgba, alpha=True):
    """RGBA pixels as a Netpbm PAM file (bytes): RGB_ALPHA, or RGB without the alpha"""
    p = np.asarray(pix_rgba, np.uint8)
    ih, iw = p.shape[:2]
    hdr = "P7\nWIDTH %d\nHEIGHT %d\nDEPTH %d\nMAXVAL 255\nTUPLTYPE %s\nENDHDR\n" % (iw, ih, 4 if alpha else 3, "RGB_ALPHA" if alpha else "RGB")
    return hdr.encode() + (p if alpha else p[:, :, :3]).tobytes()
