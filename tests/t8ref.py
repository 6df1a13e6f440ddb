"""Reference of the per-macroblock transform size choice (cfg.transform8x8 = 2, include/mi355enc.h): the luma prediction of an inter macroblock and
the rule the fused P stage applies to its residual.  numpy only; written from the standard and the rule as documented, not from the kernel.

The rule: D = source - prediction (16x16); raw4 = sum over the sixteen 4x4 blocks of sum |H4 D_b H4^T|, raw8 = sum over the four 8x8 blocks of
sum |H8 D_b H8^T| (Hadamard matrices of order 4 and 8, entries +-1, unnormalised); the 8x8 transform iff (raw8 + 2) >> 2 < raw4 >> 1, a tie keeps 4x4."""
import numpy as np

TAPS = np.array([1, -5, 20, 20, -5, 1], np.int64)


def hadamard(n):
    h = np.array([[1]], np.int64)
    while h.shape[0] < n:
        h = np.block([[h, h], [h, -h]])
    return h


H4, H8 = hadamard(4), hadamard(8)


def luma_pred(ref, x0, y0, mvx, mvy):
    """Luma prediction of the 16x16 block at (x0, y0) for the quarter-sample vector (mvx, mvy) (H.264 8.4.2.2.1: six-tap half samples, quarter samples
    averaged from their two nearest neighbours; reference coordinates clamped to the picture).  -> (16, 16) uint8"""
    H, W = ref.shape
    r = ref.astype(np.int64)
    xi, yi, xf, yf = x0 + (mvx >> 2), y0 + (mvy >> 2), mvx & 3, mvy & 3

    def full(dy, dx):  # integer samples G(x + dx, y + dy) for the 16x16 block, each offset a shift of the whole block
        ys = np.clip(yi + dy + np.arange(16), 0, H - 1)[:, None]
        xs = np.clip(xi + dx + np.arange(16), 0, W - 1)[None, :]
        return r[ys, xs]

    def clip1(v):
        return np.clip(v, 0, 255)

    def b1(dy=0, dx=0):  # horizontal six-tap sum at half-sample column x + 1/2
        return sum(TAPS[k] * full(dy, dx + k - 2) for k in range(6))

    def h1(dy=0, dx=0):  # vertical six-tap sum at half-sample row y + 1/2
        return sum(TAPS[k] * full(dy + k - 2, dx) for k in range(6))

    def j1():
        return sum(TAPS[k] * b1(k - 2, 0) for k in range(6))

    G = full(0, 0)
    b = clip1((b1() + 16) >> 5)
    h = clip1((h1() + 16) >> 5)
    j = clip1((j1() + 512) >> 10)
    s = clip1((b1(1, 0) + 16) >> 5)  # b one row down
    m = clip1((h1(0, 1) + 16) >> 5)  # h one column right

    def avg(p, q):
        return (p + q + 1) >> 1

    table = {
        (0, 0): lambda: G, (0, 1): lambda: avg(G, h), (0, 2): lambda: h, (0, 3): lambda: avg(full(1, 0), h),
        (1, 0): lambda: avg(G, b), (1, 1): lambda: avg(b, h), (1, 2): lambda: avg(h, j), (1, 3): lambda: avg(h, s),
        (2, 0): lambda: b, (2, 1): lambda: avg(b, j), (2, 2): lambda: j, (2, 3): lambda: avg(j, s),
        (3, 0): lambda: avg(full(0, 1), b), (3, 1): lambda: avg(b, m), (3, 2): lambda: avg(j, m), (3, 3): lambda: avg(m, s),
    }
    return table[(xf, yf)]().astype(np.uint8)


def _had_sum(d, hm):
    n = hm.shape[0]
    tot = 0
    for by in range(0, 16, n):
        for bx in range(0, 16, n):
            tot += int(np.abs(hm @ d[by:by + n, bx:bx + n] @ hm.T).sum())
    return tot


def raw4(d):
    """sum over the sixteen 4x4 blocks of sum |H4 d H4^T| (unhalved SATD)"""
    return _had_sum(np.asarray(d, np.int64), H4)


def raw8(d):
    """sum over the four 8x8 blocks of sum |H8 d H8^T| (unhalved SA8D)"""
    return _had_sum(np.asarray(d, np.int64), H8)


def decide_residual(d):
    """True: the 8x8 transform for residual d (16x16)"""
    return (raw8(d) + 2) >> 2 < raw4(d) >> 1


def decide(src_y, ref_y, mbx, mby, mvx, mvy):
    """The choice for the inter macroblock (mbx, mby) coded with vector (mvx, mvy) against ref_y: True = 8x8."""
    x0, y0 = 16 * mbx, 16 * mby
    d = src_y[y0:y0 + 16, x0:x0 + 16].astype(np.int64) - luma_pred(ref_y, x0, y0, int(mvx), int(mvy)).astype(np.int64)
    return decide_residual(d)
