"""The motion-compensated form of the temporal noise filter restated in plain numpy integers on top of tests/denoiseref.py: the key of a
candidate, the search per aligned 8 x 8 luma block over the history's codes, one step with displaced history reads (the chroma's by H.264's chroma prediction
for a whole-sample luma vector), and a chain with a range per picture.  Nothing here calls the library."""
import numpy as np

from tests import denoiseref as D

MAX_RANGE = 16
MAX_COST = 64 * 255


def key(cost, dx, dy, s):
    """the unsigned 32-bit word a candidate is ranked by: the cost with lambda = 4 s per sample of vector length in the high half, a rank unique per vector
    (shorter first, then by dy, then by dx) in the low half"""
    n = abs(int(dx)) + abs(int(dy))
    return ((int(cost) + 4 * int(s) * n) << 16) | (n * 1089 + (int(dy) + 16) * 33 + int(dx) + 16)


def _visible_blocks(H, W, vh, vw):
    """(H / 8, W / 8) bool: the aligned 8 x 8 blocks with at least one visible sample"""
    return np.outer(np.arange(H // 8) * 8 < vh, np.arange(W // 8) * 8 < vw)


def search(y, hy, s, rng, visible=None):
    """y (H, W) uint8, hy its history (uint16), s the strength that builds B, rng 1 .. 16.  Returns (vec (H / 8, W / 8, 2) int8 as (dx, dy), M (H / 8, W / 8)
    uint16): per block with a visible sample the candidate with the smallest key among those whose displaced block lies inside the surface, and its cost;
    zeros for a block without one."""
    H, W = y.shape
    vw, vh = visible if visible is not None else (W, H)
    c = y.astype(np.int16)
    # (the apron of zeros is read only by candidates that `ok` leaves out)
    q = np.pad(((hy.astype(np.int64) + 8) >> 4).astype(np.int16), rng)
    Y, X = np.arange(H // 8)[:, None] * 8, np.arange(W // 8)[None, :] * 8
    best = np.full((H // 8, W // 8), 1 << 32, dtype=np.int64)
    for dy in range(-rng, rng + 1):
        for dx in range(-rng, rng + 1):
            ok = (X + dx >= 0) & (X + dx <= W - 8) & (Y + dy >= 0) & (Y + dy <= H - 8)
            if not ok.any():
                continue
            cost = np.abs(c - q[rng + dy:rng + dy + H, rng + dx:rng + dx + W]).reshape(H // 8, 8, W // 8, 8).sum(axis=(1, 3), dtype=np.int64)
            n = abs(dx) + abs(dy)
            k = ((cost + 4 * s * n) << 16) | (n * 1089 + (dy + 16) * 33 + dx + 16)
            best = np.where(ok & (k < best), k, best)
    rank = (best & 0xFFFF) % 1089
    dy, dx = rank // 33 - 16, rank % 33 - 16
    m = (best >> 16) - 4 * s * (np.abs(dx) + np.abs(dy))
    vis = _visible_blocks(H, W, vh, vw)
    vec = np.stack([np.where(vis, dx, 0), np.where(vis, dy, 0)], axis=2).astype(np.int8)
    return vec, np.where(vis, m, 0).astype(np.uint16)


def displaced_luma(hy, vec):
    """H(x + dx, y + dy) with the vector of the sample's block"""
    H, W = hy.shape
    dx = np.repeat(np.repeat(vec[:, :, 0].astype(np.int64), 8, axis=0), 8, axis=1)
    dy = np.repeat(np.repeat(vec[:, :, 1].astype(np.int64), 8, axis=0), 8, axis=1)
    yy, xx = np.mgrid[0:H, 0:W]
    return hy.astype(np.int64)[yy + dy, xx + dx]


def displaced_chroma(huv, vec):
    """the chroma history a block's 4 x 4 pairs are filtered against: whole pairs at (dx >> 1, dy >> 1), the rounded mean of two along an odd axis, of four with
    both odd; per byte of the pair"""
    Hc, W = huv.shape
    h = huv.astype(np.int64)
    dx = np.repeat(np.repeat(vec[:, :, 0].astype(np.int64), 4, axis=0), 8, axis=1)
    dy = np.repeat(np.repeat(vec[:, :, 1].astype(np.int64), 4, axis=0), 8, axis=1)
    ix, iy, fx, fy = dx >> 1, dy >> 1, dx & 1, dy & 1
    yy, xx = np.mgrid[0:Hc, 0:W]
    r0, x0 = yy + iy, xx + 2 * ix
    # (where an axis is even its second neighbour is never used: keep the index in place there so that it stays inside)
    r1, x1 = r0 + fy, x0 + 2 * fx
    a, b, c, d = h[r0, x0], h[r0, x1], h[r1, x0], h[r1, x1]
    return np.where((fx == 1) & (fy == 1), (a + b + c + d + 2) >> 2, np.where(fx == 1, (a + b + 1) >> 1, np.where(fy == 1, (a + c + 1) >> 1, a)))


def step(y, uv, hy, huv, luma, chroma, rng=0, visible=None, prev=None, vectors=False):
    """denoiseref.step with a search range: 0, or a picture on which nothing is filtered (priming), is that step itself.  Otherwise the block measure M is the
    cost of the block's vector, the luma is filtered against H(x + dx, y + dy) and the chroma against displaced_chroma.  vectors: returns (vec, M) behind the four
    planes (None, None where no search ran)."""
    H, W = y.shape
    vw, vh = visible if visible is not None else (W, H)
    if prev is None:
        prev = (luma if hy is not None else 0, chroma if huv is not None else 0)
    lf, cf = luma > 0 and prev[0] > 0, chroma > 0 and prev[1] > 0
    if rng == 0 or not (lf or cf):
        out = D.step(y, uv, hy, huv, luma, chroma, visible, prev)
        return out + (None, None) if vectors else out
    B, PL, PC = D.tables(luma, chroma)
    c, cc = y.astype(np.int64), uv.astype(np.int64)
    vec, m = search(y, hy, luma if luma else chroma, rng, (vw, vh))
    b = np.repeat(np.repeat(B.astype(np.int64)[np.minimum(255, m.astype(np.int64) >> 4)], 8, axis=0), 8, axis=1)
    oy, nhy = D._filter(c, displaced_luma(hy, vec), b, PL) if lf else (c, 16 * c)
    nhy = D._replicate(nhy, vh, vw, False).astype(np.uint16)
    oy = D._replicate(oy, vh, vw, False) if lf else c
    ouv, nhuv = cc, None
    if chroma:
        ouv, nhuv = D._filter(cc, displaced_chroma(huv, vec), b[0::2], PC) if cf else (cc, 16 * cc)
        nhuv = D._replicate(nhuv, vh, vw, True).astype(np.uint16)
        ouv = D._replicate(ouv, vh, vw, True) if cf else cc
    out = (oy.astype(np.uint8), ouv.astype(np.uint8), nhy, nhuv)
    return out + (vec, m) if vectors else out


def chain(pictures, strengths, ranges, visible=None):
    """denoiseref.chain with a range per picture: a change of range, 0 included, keeps the history.  Returns the list of (y', uv')."""
    out, hy, huv, prev = [], None, None, (0, 0)
    for (y, uv), (l, c), r in zip(pictures, strengths, ranges):
        oy, ouv, hy, huv = step(y, uv, hy, huv, l, c, r, visible, prev)
        out.append((oy, ouv))
        prev = (l, c)
    return out
