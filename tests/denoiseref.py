"""The rule of the temporal noise filter restated in plain numpy integers: the three tables, one step on NV12 surfaces of the coded size
and their histories (uint16, sixteenths of a code), priming, the margins' rule, and a chain over a sequence of pictures.  Nothing here calls the library."""
import numpy as np

MAX = 32


def sample_table(s):
    """P_s[a] = clip(0, 224, floor(224 (3 s - a) / (2 s))) (numpy's // is floor division); s = 0: zeros"""
    a = np.arange(256, dtype=np.int64)
    return (np.clip((224 * (3 * s - a)) // (2 * s), 0, 224) if s > 0 else 0 * a).astype(np.uint8)


def block_table(s):
    """B[i] = clip(0, 255, floor(255 (6 s - i) / (4 s)))"""
    i = np.arange(256, dtype=np.int64)
    return (np.clip((255 * (6 * s - i)) // (4 * s), 0, 255) if s > 0 else 0 * i).astype(np.uint8)


def tables(luma, chroma):
    """(B, the luma's P, the chroma's P): B with the luma strength, or the chroma strength when luma is 0"""
    return block_table(luma if luma else chroma), sample_table(luma), sample_table(chroma)


def _filter(c, h, b, p):
    """c: codes, h: histories, b: the block weight per sample (all int64, one shape); p: the plane's table.  Returns (out, H')."""
    d = np.abs(c - ((h + 8) >> 4))
    k = (b * p.astype(np.int64)[d] + 128) >> 8
    hn = 16 * c + ((k * (h - 16 * c) + 128) >> 8)
    return (hn + 8) >> 4, hn


def _replicate(a, vh, vw, pair):
    """every 8 x 8 block (chroma: 4 rows x 4 pairs) of `a` without a visible sample takes its clamped visible position's value; partly visible ones stay"""
    H, W = a.shape[0], a.shape[1]
    rows, cols = (4, 8) if pair else (8, 8)  # (a chroma block: 4 rows of 8 bytes)
    vr, vc = (vh // 2, vw) if pair else (vh, vw)
    out = a.copy()
    y = np.arange(H)
    x = np.arange(W)
    my = (y // rows) * rows >= vr  # rows of blocks that start past the visible part
    mx = (x // cols) * cols >= vc
    sy = np.where(my, vr - 1, y)
    sx = np.where(mx, (vc - 2 + (x & 1)) if pair else vc - 1, x)  # (a chroma byte keeps its place in the pair)
    return out[np.ix_(sy, sx)]


def step(y, uv, hy, huv, luma, chroma, visible=None, prev=None):
    """One picture through the step.  y (H, W), uv (H / 2, W) uint8: the coded surfaces; hy, huv: their histories (uint16, the same shapes) or None.  luma,
    chroma: the strengths.  visible: (vw, vh), default the whole surface.  prev: the strengths of the previous picture through the step -- a plane whose strength
    was 0 there primes (out = c, H' = 16 c); default: what makes the given histories valid.  Returns (y', uv', hy', huv'): a plane with strength 0 is returned
    as it came; the chroma then has no history (None), the luma's follows the luma (16 c) while the chroma alone is filtered, for the block measure."""
    H, W = y.shape
    vw, vh = visible if visible is not None else (W, H)
    if not luma and not chroma:
        return y.copy(), uv.copy(), None, None
    if prev is None:
        prev = (luma if hy is not None else 0, chroma if huv is not None else 0)
    B, PL, PC = tables(luma, chroma)
    c, cc = y.astype(np.int64), uv.astype(np.int64)
    lf, cf = luma > 0 and prev[0] > 0, chroma > 0 and prev[1] > 0
    if lf or cf:
        h = hy.astype(np.int64)
        m = np.abs(c - ((h + 8) >> 4)).reshape(H // 8, 8, W // 8, 8).sum(axis=(1, 3))
        b = np.repeat(np.repeat(B.astype(np.int64)[np.minimum(255, m >> 4)], 8, axis=0), 8, axis=1)
    oy, nhy = _filter(c, hy.astype(np.int64), b, PL) if lf else (c, 16 * c)
    nhy = _replicate(nhy, vh, vw, False).astype(np.uint16)
    oy = _replicate(oy, vh, vw, False) if lf else c  # (priming and following do not write the surface)
    ouv, nhuv = cc, None
    if chroma:
        ouv, nhuv = _filter(cc, huv.astype(np.int64), b[0::2], PC) if cf else (cc, 16 * cc)  # (a chroma row's weight: that of the block its two luma rows lie in)
        nhuv = _replicate(nhuv, vh, vw, True).astype(np.uint16)
        ouv = _replicate(ouv, vh, vw, True) if cf else cc
    return oy.astype(np.uint8), ouv.astype(np.uint8), nhy, nhuv


def chain(pictures, strengths, visible=None):
    """A sequence of coded pictures [(y, uv), ...] through the step with a strength pair per picture, as a handle runs it.  Returns the list of (y', uv')."""
    out, hy, huv, prev = [], None, None, (0, 0)
    for (y, uv), (l, c) in zip(pictures, strengths):
        oy, ouv, hy, huv = step(y, uv, hy, huv, l, c, visible, prev)
        out.append((oy, ouv))
        prev = (l, c)
    return out


def with_margins(y, uv, W, H):
    """visible planes y (vh, vw), uv (vh / 2, vw) inside coded surfaces of W x H, the margins replicas of the last visible row and column (chroma: pair)"""
    vh, vw = y.shape
    Y = np.pad(y, ((0, H - vh), (0, W - vw)), mode="edge")
    c = uv.reshape(vh // 2, vw // 2, 2)
    C = np.pad(c, ((0, (H - vh) // 2), (0, (W - vw) // 2), (0, 0)), mode="edge").reshape(H // 2, W)
    return Y, C


def psnr(a, b):
    e = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 99.0 if e == 0 else 10 * np.log10(255.0 ** 2 / e)
