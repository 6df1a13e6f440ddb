"""numpy / Python-integer restatement of the electronic image stabiliser's rule, written from the rule's text:

- measured on the luma of the submitted picture at the input size w x h, the whole picture;
- projections: horizontal band k = rows [k h // 4, (k + 1) h // 4) gives the column sums C_k[x]; vertical band k = columns [k w // 4, (k + 1) w // 4)
  gives the row sums R_k[y];
- vote of a projection p (length n) against the previous picture's q: cost(d) = sum_{x = range}^{n - range - 1} |p[x] - q[x - d]| for d in -range .. range
  (exact integers); the d of the smallest cost, valid only if that minimum is unique and |d| < range;
- motion: the lower median of the valid votes of an axis' four bands, sorted v[(count - 1) // 2]; 0 with none;
- trajectory per axis, S in 1/256 sample: S = ((S (256 - leak)) >> 8) + 256 m with a floor shift, S = clip(S, 256 lo, 256 hi),
  o = clip(2 ((S + 256) >> 9), lo, hi); lo = -min(margin, crop origin), hi = min(margin, input - crop origin - crop size), both even towards zero;
- the first picture primes: m = 0, S = 0, o = 0, and its projections become "previous";
- the offset displaces every tap index and the clamp rectangle of the tables of the crop AS SET (tests/geomref.py): luma by (ox, oy), chroma columns by
  ox / 2, 4:2:0 chroma rows by oy / 2, 4:2:2 chroma rows by oy.
"""
import numpy as np

from tests import geomref as G

KEYS = ("mx", "my", "votes_x", "votes_y", "ox", "oy", "sx", "sy")


def project(luma):
    """(C (4, w), R (4, h)) uint32 of a 2-D luma array"""
    y = np.asarray(luma).astype(np.int64)
    h, w = y.shape
    c = np.stack([y[k * h // 4:(k + 1) * h // 4].sum(axis=0) for k in range(4)])
    r = np.stack([y[:, k * w // 4:(k + 1) * w // 4].sum(axis=1) for k in range(4)])
    return c.astype(np.uint32), r.astype(np.uint32)


def costs(p, q, rng):
    p, q = np.asarray(p).astype(np.int64), np.asarray(q).astype(np.int64)
    n = p.size
    assert q.size == n and rng >= 1 and n >= 4 * rng
    x = np.arange(rng, n - rng)
    return [int(np.abs(p[x] - q[x - d]).sum()) for d in range(-rng, rng + 1)]


def vote(p, q, rng):
    """(valid, d): d is the first shift of the smallest cost either way"""
    c = costs(p, q, rng)
    best = min(c)
    d = c.index(best) - rng
    return c.count(best) == 1 and abs(d) < rng, d


def motion(votes):
    v = sorted(votes)
    return v[(len(v) - 1) // 2] if v else 0


def bounds(margin, origin, size, total):
    lo, hi = min(margin, origin), min(margin, total - origin - size)
    return -(max(lo, 0) // 2 * 2), max(hi, 0) // 2 * 2


def step(S, m, leak, lo, hi):
    """-> (S, o); Python's >> on integers is the floor shift the rule asks for"""
    S = ((S * (256 - leak)) >> 8) + 256 * m
    S = min(max(S, 256 * lo), 256 * hi)
    return S, min(max(2 * ((S + 256) >> 9), lo), hi)


def match(prev, cur, rng, leak, bnd, state, prime=False):
    """one picture's record from the previous and the current sums; bnd = (lo_x, hi_x, lo_y, hi_y), state = (Sx, Sy)"""
    if prime:
        return dict.fromkeys(KEYS, 0)
    vx = [vote(cur[0][k], prev[0][k], rng) for k in range(4)]
    vy = [vote(cur[1][k], prev[1][k], rng) for k in range(4)]
    gx, gy = [d for ok, d in vx if ok], [d for ok, d in vy if ok]
    mx, my = motion(gx), motion(gy)
    sx, ox = step(state[0], mx, leak, bnd[0], bnd[1])
    sy, oy = step(state[1], my, leak, bnd[2], bnd[3])
    return dict(mx=mx, my=my, votes_x=len(gx), votes_y=len(gy), ox=ox, oy=oy, sx=sx, sy=sy)


class Stabilizer:
    """the stream's state: feed(luma, crop) -> the picture's record"""

    def __init__(self, rng, leak, margin_x, margin_y, in_w, in_h):
        assert in_w >= 4 * rng and in_h >= 4 * rng
        self.rng, self.leak, self.margin, self.size = rng, leak, (margin_x, margin_y), (in_w, in_h)
        self.prev, self.state = None, (0, 0)

    def feed(self, luma, crop):
        cx, cy, cw, ch = crop
        cur = project(luma)
        bnd = bounds(self.margin[0], cx, cw, self.size[0]) + bounds(self.margin[1], cy, ch, self.size[1])
        rec = match(self.prev, cur, self.rng, self.leak, bnd, self.state, prime=self.prev is None)
        self.prev, self.state = cur, (rec["sx"], rec["sy"])
        return rec


def _moved(tab, o):
    return [(f + o, q) for f, q in tab]


def to_nv12(fmt, planes, in_w, in_h, crop, dst, tw, th, ox, oy, border=G.BLACK):
    """geomref.to_nv12 with the displaced base tables: the tables of `crop`, every index and the clamp rectangle moved by the (even) offset"""
    assert G.valid(in_w, in_h, crop, dst, tw, th) and ox % 2 == 0 and oy % 2 == 0
    cx, cy, cw, ch = crop
    dx, dy, dw, dh = dst
    assert 0 <= cx + ox and cx + cw + ox <= in_w and 0 <= cy + oy and cy + ch + oy <= in_h
    y, u, v = G.components(fmt, planes, in_w, in_h)
    hx, hy = ox // 2, oy // 2
    ty = G.resample(y, _moved(G.table(cx, cw, dw, G.LUMA), ox), _moved(G.table(cy, ch, dh, G.LUMA), oy), cx + ox, cx + cw - 1 + ox, cy + oy, cy + ch - 1 + oy)
    tab_ch = _moved(G.table(cx, cw, dw, G.CHROMA_H), hx)
    if fmt in (G.FMT_YUY2, G.FMT_UYVY):
        tab_cv, r0, r1 = _moved(G.table(cy, ch, dh, G.CHROMA_V422), oy), cy + oy, cy + ch - 1 + oy
    else:
        tab_cv, r0, r1 = _moved(G.table(cy, ch, dh, G.CHROMA_V), hy), cy // 2 + hy, (cy + ch) // 2 - 1 + hy
    tu = G.resample(u, tab_ch, tab_cv, cx // 2 + hx, (cx + cw) // 2 - 1 + hx, r0, r1)
    tv = G.resample(v, tab_ch, tab_cv, cx // 2 + hx, (cx + cw) // 2 - 1 + hx, r0, r1)
    oy_, ou, ov = np.full((th, tw), border[0], np.uint8), np.full((th // 2, tw // 2), border[1], np.uint8), np.full((th // 2, tw // 2), border[2], np.uint8)
    oy_[dy:dy + dh, dx:dx + dw] = ty
    ou[dy // 2:(dy + dh) // 2, dx // 2:(dx + dw) // 2] = tu
    ov[dy // 2:(dy + dh) // 2, dx // 2:(dx + dw) // 2] = tv
    return G.nv12_surfaces(oy_, ou, ov)


def world(seed, w=512, h=384):
    """a seeded "world": 4 x 4 noise blocks, luma and interleaved chroma (NV12 planes of w x h)"""
    rng = np.random.default_rng(seed)
    y = np.kron(rng.integers(16, 236, (h // 4, w // 4), dtype=np.uint8), np.ones((4, 4), np.uint8))
    uv = np.kron(rng.integers(64, 192, (h // 8, w // 8, 2), dtype=np.uint8), np.ones((4, 4, 1), np.uint8)).reshape(h // 2, w)
    return y, uv


def cut(wld, x, y, w, h, seed):
    """the w x h NV12 window of the world at (x, y), with +-3 of fresh noise on every luma sample"""
    wy, wuv = wld
    n = np.random.default_rng(seed).integers(-3, 4, (h, w))
    ly = np.clip(wy[y:y + h, x:x + w].astype(np.int64) + n, 0, 255).astype(np.uint8)
    cx, cy = x // 2 * 2, y // 2
    return np.ascontiguousarray(ly), np.ascontiguousarray(wuv[cy:cy + h // 2, cx:cx + w])


CEIL = 2048 * 255  # the largest sum: a band of 2048 rows of 255


def match_cases():
    """[(name, prev, cur, range, leak, bounds, state)]: projection sets (prev, cur = (C (4, w), R (4, h))) for the vote, the medians and the step -- known
    shifts, flat bands and exact ties, minima on the window's edge, n = 4 range exactly, and sums at their ceiling (the 33-bit cost) with range 32"""
    rng = np.random.default_rng(2600)

    def rand(n, top=CEIL):
        return rng.integers(0, top + 1, n).astype(np.uint32)

    def pair(n, d, top=CEIL):  # cur[x] = prev[x - d] wherever the vote looks
        q = rand(n, top)
        return q, np.roll(q, d)

    def build(w, h, cols, rows):
        pc, cc = zip(*cols)
        pr, cr = zip(*rows)
        return (np.stack(pc), np.stack(pr)), (np.stack(cc), np.stack(cr))

    out = []
    w, h = 64, 48
    prev, cur = build(w, h, [pair(w, d) for d in (2, 2, -1, 2)], [pair(h, d) for d in (3, -3, 0, 1)])
    out.append(("shifts", prev, cur, 4, 16, (-16, 16, -16, 16), (-300, 700)))
    flat = (np.full(w, 1234, np.uint32), np.full(w, 1234, np.uint32))
    alt = (np.tile(np.array([0, 9], np.uint32), w // 2), np.tile(np.array([0, 9], np.uint32), w // 2))
    fr = (np.full(h, 77, np.uint32), np.full(h, 77, np.uint32))
    prev, cur = build(w, h, [flat, alt, pair(w, 1), pair(w, -2)], [fr, fr, fr, fr])
    out.append(("flat-and-ties", prev, cur, 4, 0, (0, 0, 0, 0), (0, 0)))
    prev, cur = build(w, h, [pair(w, d) for d in (4, -4, 4, 3)], [pair(h, -4) for _ in range(4)])
    out.append(("edge", prev, cur, 4, 255, (-16, 0, 0, 6), (-4000, 1500)))
    prev, cur = build(32, 32, [pair(32, d, 4000) for d in (7, 7, -7, 7)], [pair(32, d, 4000) for d in (-1, -1, 6, 8)])
    out.append(("n=4range", prev, cur, 8, 1, (-1024, 1024, -2, 0), (-262144, 100)))
    w, h = 8192, 128
    a = np.tile(np.array([0, CEIL], np.uint32), w // 2)
    two = lambda d: (lambda q: (q, np.roll(q, d)))((rng.integers(0, 2, w) * CEIL).astype(np.uint32))
    prev, cur = build(w, h, [(CEIL - a, a), (a, a), two(5), two(-7)], [pair(h, d) for d in (31, -31, 0, 1)])
    out.append(("ceiling", prev, cur, 32, 254, (-32, 32, -1024, 1024), (8000, -262144)))
    return out


EXPECT = {"shifts": (2, 0, 4, 4), "flat-and-ties": (-2, 0, 2, 0), "edge": (3, 0, 1, 0), "n=4range": (7, -1, 4, 3), "ceiling": (-7, 0, 2, 4)}  # mx, my, votes_x, votes_y


# the scripted shake of the stream tests, as motion of the content per picture (the window moves the other way): jitter of up to +-7, then a steady pan that
# drives the offset into its bound
SCRIPT = [(0, 0), (5, -3), (-7, 6), (3, -7), (-6, 2), (7, 5), (-2, -4), (-5, 6), (4, -3), (4, -3), (4, -3), (4, -3), (4, -3), (4, -3)]


def clip(in_w=160, in_h=96, seed=2601, script=SCRIPT):
    """NV12 pictures of in_w x in_h cut from a world along SCRIPT"""
    wld = world(seed)
    x, y, pics = 200, 150, []
    for i, (mx, my) in enumerate(script):
        x, y = x - mx, y - my
        pics.append(cut(wld, x, y, in_w, in_h, seed + 1 + i))
    return pics


def run(lumas, setting, crops, in_w, in_h):
    """the records of a stream of luma planes: setting = (range, leak, margin_x, margin_y); crops: one rectangle or one per picture"""
    st = Stabilizer(*setting, in_w, in_h)
    return [st.feed(y[:in_h, :in_w], crops[i] if isinstance(crops, list) else crops) for i, y in enumerate(lumas)]
