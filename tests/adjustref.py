"""The rule of the picture controls restated in plain numpy integers: the luma table for gamma 1000, the double model of the table for any
gamma and of the chroma rotation, and the step itself on NV12 surfaces of the coded size -- table, rotation, 3 x 3 unsharp mask, clamped to the visible part of
the picture rectangle, margins as replicas.  Nothing here calls the library."""
import numpy as np

NEUTRAL = dict(brightness=0, contrast=1000, saturation=1000, hue=0, gamma=1000, sharpen=0, sharpen_threshold=0)
RANGES = dict(brightness=(-1000, 1000), contrast=(0, 2000), saturation=(0, 2000), hue=(-1000, 1000), gamma=(100, 10000), sharpen=(-16, 64), sharpen_threshold=(0, 32))


def params(**kw):
    a = dict(NEUTRAL)
    a.update(kw)
    return a


def black_scale(full_range):
    return (0, 255) if full_range else (16, 219)


def luma_table_int(a, full_range):
    """gamma 1000: integers only (numpy's // is floor division)"""
    assert a["gamma"] == 1000
    B, S = black_scale(full_range)
    v = np.arange(256, dtype=np.int64)
    return np.clip(B + (2 * ((v - B) * a["contrast"] + a["brightness"] * S) + 1000) // 2000, 0, 255).astype(np.uint8)


def luma_model(a, full_range):
    """the table before rounding, in double: float64 (256,)"""
    B, S = black_scale(full_range)
    t = (np.arange(256, dtype=np.float64) - B) / S
    inside = (t >= 0.0) & (t <= 1.0)
    t = np.where(inside, np.power(np.clip(t, 0.0, 1.0), 1000.0 / a["gamma"]), t)
    return B + S * (t * a["contrast"] / 1000.0 + a["brightness"] / 1000.0)


def chroma_model(a):
    """(cu, su) before rounding, in double"""
    g, ang = 4096.0 * a["saturation"] / 1000.0, np.pi * a["hue"] / 1000.0
    return g * np.cos(ang), g * np.sin(ang)


def rotate(uv, chroma):
    """interleaved Cb Cr bytes (.., 2 n) through the rotation {cu, su}"""
    cu, su = int(chroma[0]), int(chroma[1])
    c = uv.astype(np.int64) - 128
    a, b = c[..., 0::2], c[..., 1::2]
    out = np.empty_like(c)
    out[..., 0::2] = 128 + ((cu * a + su * b + 2048) >> 12)
    out[..., 1::2] = 128 + ((-su * a + cu * b + 2048) >> 12)
    return np.clip(out, 0, 255).astype(np.uint8)


def binomial_sum(y):
    """sum of the 3 x 3 weights 1 2 1 / 2 4 2 / 1 2 1 over y with its edge samples repeated: int64, y's shape"""
    p = np.pad(y.astype(np.int64), 1, mode="edge")
    h = p[:, :-2] + 2 * p[:, 1:-1] + p[:, 2:]
    return h[:-2] + 2 * h[1:-1] + h[2:]


def sharpen(y, amount, threshold):
    """the unsharp mask on a whole visible luma picture (uint8 2-D), neighbours clamped at its edge"""
    c = y.astype(np.int64)
    d = 16 * c - binomial_sum(y)
    out = np.clip(c + ((amount * d + 128) >> 8), 0, 255)
    if amount > 0:
        out = np.where(np.abs(d) <= 16 * threshold, c, out)
    return out.astype(np.uint8)


def apply(y, uv, a, luma, chroma, rect=None, visible=None):
    """The step on coded NV12 surfaces y (H, W), uv (H / 2, W) with the tables the library returned.  rect: x0, x1, y0, y1 (even), the part that is picture --
    reaching the surfaces' edge where it reaches the visible picture's; visible: (vw, vh).  Returns new arrays; everything outside rect keeps its bytes."""
    H, W = y.shape
    x0, x1, y0, y1 = rect if rect is not None else (0, W, 0, H)
    vw, vh = visible if visible is not None else (W, H)
    vx1, vy1 = min(x1, vw), min(y1, vh)
    oy, ouv = y.copy(), uv.copy()
    t = np.asarray(luma, np.uint8)[y[y0:y1, x0:x1]]
    if a["sharpen"]:
        vis = sharpen(t[:vy1 - y0, :vx1 - x0], a["sharpen"], a["sharpen_threshold"])
        t = np.pad(vis, ((0, y1 - vy1), (0, x1 - vx1)), mode="edge")  # a margin sample is the result of its clamped visible position
    oy[y0:y1, x0:x1] = t
    ouv[y0 // 2:y1 // 2, x0:x1] = rotate(uv[y0 // 2:y1 // 2, x0:x1], chroma)
    return oy, ouv


def with_margins(y, uv, W, H):
    """visible planes y (vh, vw), uv (vh / 2, vw) inside coded surfaces of W x H, the margins replicas of the last visible row and column (chroma: pair)"""
    vh, vw = y.shape
    Y = np.pad(y, ((0, H - vh), (0, W - vw)), mode="edge")
    c = uv.reshape(vh // 2, vw // 2, 2)
    C = np.pad(c, ((0, (H - vh) // 2), (0, (W - vw) // 2), (0, 0)), mode="edge").reshape(H // 2, W)
    return Y, C
