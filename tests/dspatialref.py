"""The spatial noise filter and its noise estimate restated in numpy integers: the tables, the two stencils with their edge rule, the
block measure, the decision and the chain a handle runs over a sequence of pictures.  The third statement of the rule beside dspatial_host.h / dspatial_host.c
and k_dspatial.hip; the GPU is held to this one bit for bit."""
import numpy as np

MAX = 32
NAMES = ("luma", "chroma", "auto_gain", "percentile", "speed")
DEFAULT = dict(luma=0, chroma=0, auto_gain=0, percentile=25, speed=32)
REC = ("candidates", "voters", "v", "valid", "x", "s_luma", "s_chroma")
ZERO = dict.fromkeys(REC, 0)
W5, W3 = (1, 4, 6, 4, 1), (1, 2, 1)


def params(a=None, **kw):
    """the full setting of a dict; one that neither filters nor measures is off: the defaults"""
    p = dict(DEFAULT, **dict(a or {}, **kw))
    return p if active(p) else dict(DEFAULT)


def active(p):
    return p["auto_gain"] > 0 or p["luma"] > 0 or p["chroma"] > 0


def black_scale(full):
    return (0, 255) if full else (16, 219)


def weight_table(s):
    """R_s[a] = clip(0, 16, floor(16 (3 s - a) / (2 s))) (numpy's // is floor division); s = 0: zeros"""
    a = np.arange(256, dtype=np.int64)
    return np.clip((16 * (3 * s - a)) // (2 * s), 0, 16) if s > 0 else 0 * a


def filter_table(s):
    """F_s[a] = a R_s[a]"""
    return np.arange(256, dtype=np.int64) * weight_table(s)


def _signed(s):
    d = np.arange(-255, 256, dtype=np.int64)
    return np.sign(d) * filter_table(s)[np.abs(d)]


def _clamped(n0, n1, size, step):
    """positions n0 .. n1 - 1 clamped into 0 .. size - 1, by groups of `step` (a chroma byte stays a Cb or a Cr)"""
    j = np.arange(n0, n1)
    p = j & (step - 1)
    return np.clip(j - p, 0, size - step) + p


def _plane(src, x0, x1, y0, y1, vx1, vy1, s, step, rad):
    """one plane: bytes x0 .. x1 - 1 of rows y0 .. y1 - 1, visible up to (vx1, vy1); step 1 / radius 2: luma, step 2 / radius 1: the interleaved chroma plane"""
    w, shift = (W5, 12) if rad == 2 else (W3, 8)
    V = src[y0:vy1, x0:vx1].astype(np.int64)
    h, wd = V.shape
    P = V[np.clip(np.arange(-rad, h + rad), 0, h - 1)][:, _clamped(-2, wd + 2, wd, step)]  # (the halo is two bytes either way)
    T = _signed(s)
    total, lo, hi = np.zeros_like(V), V.copy(), V.copy()
    for dy in range(-rad, rad + 1):
        for dx in range(-rad, rad + 1):
            n = P[rad + dy:rad + dy + h, 2 + step * dx:2 + step * dx + wd]
            total += w[dy + rad] * w[dx + rad] * T[n - V + 255]
            lo, hi = np.minimum(lo, n), np.maximum(hi, n)
    assert np.abs(total).max(initial=0) < 1 << 21
    out = V + ((total + (1 << (shift - 1))) >> shift)
    assert (out >= lo).all() and (out <= hi).all()  # between the smallest and the largest sample of the window: no clip
    dst = src.copy()
    dst[y0:y1, x0:x1] = out[np.clip(np.arange(y1 - y0), 0, h - 1)][:, _clamped(0, x1 - x0, wd, step)].astype(np.uint8)
    return dst


def apply(y, uv, s_luma, s_chroma, rect=None, visible=None):
    """The filter on coded surfaces y (H, W) / uv (H / 2, W).  A strength of None leaves its plane alone (manual mode's 0); 0 copies it, margins replicated
    (automatic mode's 0).  rect: (x0, x1, y0, y1), default the whole surface; visible: (vw, vh), default the whole surface.  Returns (y', uv')."""
    H, W = y.shape
    x0, x1, y0, y1 = rect or (0, W, 0, H)
    vw, vh = visible or (W, H)
    vx1, vy1 = min(x1, vw), min(y1, vh)
    oy = y.copy() if s_luma is None else _plane(y, x0, x1, y0, y1, vx1, vy1, s_luma, 1, 2)
    ouv = uv.copy() if s_chroma is None else _plane(uv, x0, x1, y0 // 2, y1 // 2, (vx1 + 1) & ~1, (vy1 + 1) >> 1, s_chroma, 2, 1)
    return oy, ouv


def blocks(rect, visible):
    """the candidates: first block column, their count per row, first block row, their rows"""
    x0, x1, y0, y1 = rect
    vx1, vy1 = min(x1, visible[0]), min(y1, visible[1])
    bx0, by0 = (x0 + 7) >> 3, (y0 + 7) >> 3
    return bx0, max(0, (vx1 >> 3) - bx0), by0, max(0, (vy1 >> 3) - by0)


def block_bins(y, rect=None, visible=None):
    """(bin, sample sum) per candidate block, (brows, bcols) each"""
    H, W = y.shape
    bx0, bcols, by0, brows = blocks(rect or (0, W, 0, H), visible or (W, H))
    b = y[8 * by0:8 * (by0 + brows), 8 * bx0:8 * (bx0 + bcols)].astype(np.int64).reshape(brows, 8, bcols, 8).transpose(0, 2, 1, 3)
    hd = b[..., :, :-2] - 2 * b[..., :, 1:-1] + b[..., :, 2:]
    L = hd[..., :-2, :] - 2 * hd[..., 1:-1, :] + hd[..., 2:, :]
    A = np.abs(L).sum(axis=(-1, -2))
    return np.minimum(255, (95 * A + 1024) >> 11), b.sum(axis=(-1, -2))


def measure(y, rect=None, visible=None, full=0):
    """dict(hist=, candidates=, voters=)"""
    bins, sums = block_bins(y, rect, visible)
    B, S = black_scale(full)
    vote = (sums >= 64 * (B + (S >> 4))) & (sums <= 64 * (B + S - (S >> 4)))
    hist = np.bincount(bins[vote].ravel(), minlength=256).astype(np.int64)
    return dict(hist=hist, candidates=int(bins.size), voters=int(vote.sum()))


def percentile_bin(hist, percentile):
    cum, N = np.cumsum(np.asarray(hist, np.int64)), int(np.sum(hist))
    return int(np.argmax(100 * cum >= percentile * N))


def decide(m, a, x=None, prime=False):
    """a picture's decision from its measurement, an automatic setting and the state going in -> (record, the state coming out)"""
    a = dict(DEFAULT, **a)
    NC, N = int(m["candidates"]), int(m["voters"])
    v = percentile_bin(m["hist"], a["percentile"])
    valid = N > 0 and 16 * N >= NC
    x = 0 if x is None else int(x)
    if prime:
        x = 256 * v if valid else 0
    elif valid:
        x += ((256 * v - x) * a["speed"]) >> 8
    x = min(max(x, 0), 65280)
    s = (x * a["auto_gain"] + 1024000) // 2048000
    return dict(candidates=NC, voters=N, v=v, valid=int(valid), x=x, s_luma=min(a["luma"], s), s_chroma=min(a["chroma"], s)), x


def chain(pictures, settings, full=0, rect=None, visible=None):
    """A sequence of coded pictures [(y, uv), ...] through the step with a setting (a dict, or None: off) per picture, as a handle runs it.  Returns the list of
    (y', uv', record)."""
    out, x, primed = [], 0, False
    for (y, uv), a in zip(pictures, settings):
        a = params(a)
        if not active(a):
            primed = False
            out.append((y.copy(), uv.copy(), dict(ZERO)))
        elif a["auto_gain"] == 0:
            primed = False
            oy, ouv = apply(y, uv, a["luma"] or None, a["chroma"] or None, rect, visible)
            out.append((oy, ouv, dict(ZERO, s_luma=a["luma"], s_chroma=a["chroma"])))
        else:
            rec, x = decide(measure(y, rect, visible, full), a, x, not primed)
            primed = True
            oy, ouv = apply(y, uv, rec["s_luma"] if a["luma"] else None, rec["s_chroma"] if a["chroma"] else None, rect, visible)
            out.append((oy, ouv, rec))
    return out


def decide_cases():
    """(name, measurement, setting, X going in or None: prime)"""
    def m(bins, NC=None):
        hist = np.bincount(np.asarray(bins, np.int64), minlength=256)
        return dict(hist=hist, candidates=len(bins) if NC is None else NC, voters=len(bins))
    noisy = m([20] * 10 + [24] * 20 + [40] * 30 + [200] * 4)
    few = m([30] * 3, NC=49)  # 16 N < NC
    on = dict(luma=32, chroma=32, auto_gain=2000)
    return [
        ("prime-valid", noisy, on, None), ("prime-invalid", few, on, None), ("prime-no-voter", m([], NC=12), on, None),
        ("invalid-while-running", few, on, 5000), ("running", noisy, on, 3000), ("running-down", noisy, on, 30000),
        ("speed-1", noisy, dict(on, speed=1), 3000), ("speed-1-down", noisy, dict(on, speed=1), 9000), ("speed-256", noisy, dict(on, speed=256), 3000),
        ("x-0", noisy, on, 0), ("x-65280", noisy, on, 65280), ("x-65280-stays", m([255] * 40), dict(on, speed=256), 65280),
        ("gain-250", noisy, dict(on, auto_gain=250), 20000), ("gain-8000", noisy, dict(on, auto_gain=8000), 20000),
        ("bounds-below-s", noisy, dict(luma=3, chroma=1, auto_gain=2000), 20000), ("bounds-above-s", noisy, dict(luma=32, chroma=31, auto_gain=1000), 2000),
        ("measure-only", noisy, dict(auto_gain=1000), None), ("percentile-1", noisy, dict(on, percentile=1), None), ("percentile-50", noisy, dict(on, percentile=50), None),
        ("flat", m([0] * 64), on, 4000),
    ]


def with_margins(y, uv, W, H):
    """visible planes y (vh, vw), uv (vh / 2, vw) inside coded surfaces of W x H, the margins replicas of the last visible row and column (chroma: pair)"""
    vh, vw = y.shape
    Y = np.pad(y, ((0, H - vh), (0, W - vw)), mode="edge")
    c = np.pad(uv.reshape(vh // 2, vw // 2, 2), ((0, H // 2 - vh // 2), (0, W // 2 - vw // 2), (0, 0)), mode="edge")
    return np.ascontiguousarray(Y), np.ascontiguousarray(c.reshape(H // 2, W))


def synthetic(w=352, h=288, sigma=0.0, seed=7):
    """the clean test picture -- its left half flat patches of 32 x 32, its right half sinusoidal texture -- plus Gaussian noise of `sigma` codes -> (clean, noisy)"""
    xx, yy = np.meshgrid(np.arange(w), np.arange(h))
    patches = 60 + 12 * (((xx // 32) * 5 + (yy // 32) * 3) % 11)
    texture = 128 + 50 * np.sin(xx / 3.1) * np.cos(yy / 4.3)
    clean = np.where(xx < w // 2, patches, texture)
    noisy = clean + sigma * np.random.default_rng(seed).standard_normal((h, w)) if sigma else clean
    return np.clip(np.rint(clean), 0, 255).astype(np.uint8), np.clip(np.rint(noisy), 0, 255).astype(np.uint8)


def noisy_clip(w, h, n, sigmas, seed=3):
    """n NV12 pictures of one drifting scene (smooth, mid-grey: every block votes) with Gaussian noise of sigmas[i] codes on luma and chroma"""
    rng = np.random.default_rng(seed)
    xx, yy = np.meshgrid(np.arange(w), np.arange(h))
    pics = []
    for i in range(n):
        base = 120 + 40 * np.sin((xx + 2 * i) / 9.0) * np.cos(yy / 7.0)
        cb = 128 + 30 * np.sin((xx[::2, ::2] + i) / 11.0)
        cr = 128 + 30 * np.cos(yy[::2, ::2] / 6.0)
        y = np.clip(np.rint(base + sigmas[i] * rng.standard_normal((h, w))), 0, 255).astype(np.uint8)
        c = np.stack([cb, cr], axis=-1) + sigmas[i] * rng.standard_normal((h // 2, w // 2, 2))
        pics.append((y, np.clip(np.rint(c), 0, 255).astype(np.uint8).reshape(h // 2, w)))
    return pics


def psnr(a, b):
    e = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 99.0 if e == 0 else 10 * np.log10(255.0 ** 2 / e)
