"""numpy restatement of automatic levels and white balance (include/mi355enc.h, mi355enc_autolevel_t), all integers: the measurement of a
picture's coded surfaces, the decision (black point, white point, chroma offsets, state), the table and the apply step, a chain of pictures as a handle runs
it, and the seeded clip and hand-made cases the tests share.  Python's >> and // are floors; where the rule divides values that are never negative that is
the rule's own division."""
import numpy as np

NAMES = ("levels", "balance", "speed", "clip_low", "clip_high", "max_gain", "reach")
DEFAULT = dict(levels=0, balance=0, speed=16, clip_low=50, clip_high=50, max_gain=2000, reach=48)
RANGES = dict(levels=(0, 1000), balance=(0, 1000), speed=(1, 256), clip_low=(0, 2000), clip_high=(0, 2000), max_gain=(1000, 8000), reach=(0, 127))
KEYS = ("lo", "hi", "voters", "du", "dv", "s_lo", "s_hi", "s_du", "s_dv", "off_u", "off_v", "valid")
ZERO = dict.fromkeys(KEYS, 0)


def params(a=None, **kw):
    """a setting's seven fields: the defaults, then a's and the keywords' on top; clip=c sets both clips"""
    src = dict(a or {}, **kw)
    if "clip" in src:
        src["clip_low"] = src["clip_high"] = src.pop("clip")
    assert not set(src) - set(NAMES), src
    return dict(DEFAULT, **src)


def active(a):
    return a["levels"] > 0 or a["balance"] > 0


def black_scale(full_range):
    return (0, 255) if full_range else (16, 219)


def with_margins(y, uv, W, H):
    """visible planes inside coded surfaces of W x H, the margins replicas of the last visible row and column (chroma: pair)"""
    vh, vw = y.shape
    Y = np.pad(y, ((0, H - vh), (0, W - vw)), mode="edge")
    c = uv.reshape(vh // 2, vw // 2, 2)
    return Y, np.pad(c, ((0, (H - vh) // 2), (0, (W - vw) // 2), (0, 0)), mode="edge").reshape(H // 2, W)


def measure(y, uv, rect=None, visible=None, full_range=0, reach=48):
    """y (H, W), uv (H / 2, W): coded surfaces; rect (x0, x1, y0, y1), default the whole surface; visible (w, h) likewise -> dict(hist, voters, su, sv, chroma)"""
    H, W = y.shape
    x0, x1, y0, y1 = rect if rect is not None else (0, W, 0, H)
    vw, vh = visible if visible is not None else (W, H)
    x1, y1 = min(x1, vw), min(y1, vh)
    B, S = black_scale(full_range)
    part = y[y0:y1, x0:x1]
    hist = np.bincount(part.reshape(-1), minlength=256).astype(np.int64)
    co = part[0::2, 0::2].astype(np.int64)  # the co-sited luma of the chroma samples that count
    c = uv.reshape(H // 2, W // 2, 2)[y0 // 2:y0 // 2 + co.shape[0], x0 // 2:x0 // 2 + co.shape[1]].astype(np.int64)
    cb, cr = c[..., 0], c[..., 1]
    vote = (co >= B + (S >> 3)) & (co <= B + S - (S >> 3)) & (np.abs(cb - 128) <= reach) & (np.abs(cr - 128) <= reach)
    return dict(hist=hist, voters=int(vote.sum()), su=int(cb[vote].sum()), sv=int(cr[vote].sum()), chroma=int(co.size))


def decide(m, a, full_range=0, state=None, prime=False):
    """-> (record, table (256,) uint8, state (Lo, Hi, Du, Dv))"""
    a = params(a)
    B, S = black_scale(full_range)
    hist = np.asarray(m["hist"], np.int64)
    N, n, NC = int(hist.sum()), int(m["voters"]), int(m["chroma"])
    cum = np.cumsum(hist)
    is_lo = 10000 * cum > a["clip_low"] * N
    is_hi = 10000 * (N - (cum - hist)) > a["clip_high"] * N
    lo = int(np.argmax(is_lo)) if is_lo.any() else 255
    hi = 255 - int(np.argmax(is_hi[::-1])) if is_hi.any() else 0
    lo, hi = min(max(lo, B), B + S), min(max(hi, B), B + S)
    valid = n > 0 and 16 * n >= NC
    du = (256 * int(m["su"])) // n - 32768 if valid else 0
    dv = (256 * int(m["sv"])) // n - 32768 if valid else 0
    if prime:
        Lo, Hi, Du, Dv = 256 * lo, 256 * hi, du, dv
    else:
        Lo, Hi, Du, Dv = [int(v) for v in state]
        Lo += ((256 * lo - Lo) * a["speed"]) >> 8
        Hi += ((256 * hi - Hi) * a["speed"]) >> 8
        if valid:
            Du += ((du - Du) * a["speed"]) >> 8
            Dv += ((dv - Dv) * a["speed"]) >> 8
    b256, t256 = 256 * B, 256 * (B + S)
    Lo, Hi = min(max(Lo, b256), t256), min(max(Hi, b256), t256)
    L = b256 + ((Lo - b256) * a["levels"]) // 1000
    T = t256 - ((t256 - Hi) * a["levels"]) // 1000
    span, smin = T - L, -((-256000 * S) // a["max_gain"])
    if span < smin:
        L = ((L + T) >> 1) - (smin >> 1)
        T = L + smin
        if L < b256:
            L, T = b256, b256 + smin
        if T > t256:
            L, T = t256 - smin, t256
        span = smin
    t = np.clip(256 * np.arange(256, dtype=np.int64) - L, 0, span)
    table = (B + (2 * t * S + span) // (2 * span)).astype(np.uint8)
    rec = dict(lo=lo, hi=hi, voters=n, du=du, dv=dv, s_lo=Lo, s_hi=Hi, s_du=Du, s_dv=Dv,
               off_u=(Du * a["balance"] + 128000) // 256000, off_v=(Dv * a["balance"] + 128000) // 256000, valid=int(valid))
    return rec, table, (Lo, Hi, Du, Dv)


def apply(y, uv, a, rec, table, rect=None):
    """in place over the whole rectangle, margins included; a plane whose correction is neutral comes back as it came"""
    a = params(a)
    H, W = y.shape
    x0, x1, y0, y1 = rect if rect is not None else (0, W, 0, H)
    oy, ouv = y.copy(), uv.copy()
    if a["levels"] > 0:
        oy[y0:y1, x0:x1] = table[y[y0:y1, x0:x1]]
    if a["balance"] > 0 and (rec["off_u"] or rec["off_v"]):
        c = ouv.reshape(H // 2, W // 2, 2)
        part = c[y0 // 2:y1 // 2, x0 // 2:x1 // 2].astype(np.int64)
        part[..., 0] -= rec["off_u"]
        part[..., 1] -= rec["off_v"]
        c[y0 // 2:y1 // 2, x0 // 2:x1 // 2] = np.clip(part, 0, 255).astype(np.uint8)
    return oy, ouv


def step(y, uv, a, full_range=0, state=None, prime=False, rect=None, visible=None):
    """one picture's coded surfaces through the three steps -> (y', uv', record, table, state)"""
    a = params(a)
    rec, table, state = decide(measure(y, uv, rect, visible, full_range, a["reach"]), a, full_range, state, prime)
    oy, ouv = apply(y, uv, a, rec, table, rect)
    return oy, ouv, rec, table, state


def chain(pictures, settings, full_range=0, rect=None, visible=None):
    """A sequence of coded pictures [(y, uv), ...] through the step with a setting (or None: off) per picture, as a handle runs it: the first picture after
    off primes.  Returns [(y', uv', record, table)]; an unprocessed picture comes back as it came with a zero record and table."""
    out, state, primed = [], None, False
    for (y, uv), a in zip(pictures, settings):
        if a is None or not active(params(a)):
            out.append((y, uv, dict(ZERO), np.zeros(256, np.uint8)))
            primed = False
            continue
        oy, ouv, rec, table, state = step(y, uv, a, full_range, state, not primed, rect, visible)
        primed = True
        out.append((oy, ouv, rec, table))
    return out


def clip(w, h, n=12, seed=7, still=False):
    """n visible NV12 pictures of a drifting scene: exposure ramping down and up again (a gain and a lift on the luma), and a chroma cast that appears at picture 5.
    still: the scene does not drift and the exposure moves a tenth as fast (a clip a temporal noise filter has something to do on)"""
    rng = np.random.default_rng(seed)
    base = rng.integers(30, 226, (h + 2 * n, w + 2 * n)).astype(np.int64)
    base[: h // 3] = base[: h // 3] // 4 + 100  # (a flatter band, so the histogram has a body and tails)
    cbase = rng.integers(108, 149, (h // 2 + n, w + 2 * n)).astype(np.int64)
    pics = []
    for i in range(n):
        k = abs(i - n // 2)  # n / 2 .. 0 .. n / 2 - 1
        gain = 700 + 10 * k if still else 400 + 100 * k  # thousandths
        d = 0 if still else i
        y = np.clip(20 + (k if still else 5 * k) + ((base[2 * d:2 * d + h, 2 * d:2 * d + w] - 30) * gain) // 1000 + rng.integers(0, 3, (h, w)), 0, 255)
        c = cbase[d:d + h // 2, 2 * d:2 * d + w].copy()
        if i >= 5:
            c[:, 0::2] += 14
            c[:, 1::2] -= 9
        pics.append((y.astype(np.uint8), np.clip(c, 0, 255).astype(np.uint8)))
    return pics


def decide_cases():
    """hand-made (name, measurement, setting, full_range, state or None (prime)) for both decide entry points"""
    def meas(hist, n=0, su=0, sv=0, nc=0):
        h = np.zeros(256, np.int64)
        for v, c in hist.items():
            h[v] = c
        return dict(hist=h, voters=n, su=su, sv=sv, chroma=nc)

    on = dict(levels=1000, balance=1000)
    cases = []
    for full in (0, 1):
        B, S = black_scale(full)
        tag = "full" if full else "limited"
        for name, v in (("B", B), ("top", B + S), ("0", 0), ("255", 255)):
            cases.append(("flat-%s-%s" % (name, tag), meas({v: 4096}, 64, 64 * 120, 64 * 140, 1024), on, full, None))
        cases.append(("spikes-" + tag, meas({40: 1000, 200: 1000}), on, full, None))
        cases.append(("clips0-" + tag, meas({3: 1, 60: 5000, 180: 5000, 250: 1}), dict(on, clip_low=0, clip_high=0), full, None))
        cases.append(("clips-" + tag, meas({3: 1, 60: 5000, 180: 5000, 250: 1}), on, full, None))
        cases.append(("one-" + tag, meas({77: 1}, 1, 130, 126, 1), on, full, None))
        cases.append(("below-" + tag, meas({0: 10, 5: 100, B // 2: 50}), on, full, (256 * (B + 20), 256 * (B + 180), 0, 0)))
        cases.append(("voters-at-" + tag, meas({100: 1600}, 100, 100 * 140, 100 * 120, 1600), on, full, None))
        cases.append(("voters-under-" + tag, meas({100: 1600}, 99, 99 * 140, 99 * 120, 1600), on, full, (256 * 90, 256 * 200, 500, -700)))
        cases.append(("no-voters-" + tag, meas({100: 1600}, 0, 0, 0, 1600), on, full, (256 * 90, 256 * 200, 500, -700)))
        for speed in (1, 256):
            cases.append(("speed%d-%s" % (speed, tag), meas({50: 900, 150: 900}, 400, 400 * 100, 400 * 150, 450), dict(on, speed=speed), full, (256 * 100, 256 * 120, -3000, 2500)))
        for g in (1000, 8000):
            cases.append(("gain%d-%s" % (g, tag), meas({90: 500, 110: 500}), dict(on, max_gain=g), full, None))
            cases.append(("gain%d-wide-%s" % (g, tag), meas({B: 500, B + S: 500}), dict(on, max_gain=g), full, None))
        for bal in (1, 250, 499, 500, 501, 999, 1000):
            cases.append(("negative-du-bal%d-%s" % (bal, tag), meas({100: 1600}, 800, 800 * 97 + 13, 800 * 121 + 5, 1600), dict(levels=300, balance=bal), full, (256 * 60, 256 * 190, -7777, -129)))
        cases.append(("levels0-" + tag, meas({100: 1600}, 800, 800 * 140, 800 * 120, 1600), dict(balance=700), full, None))
        cases.append(("balance0-" + tag, meas({70: 800, 170: 800}, 800, 800 * 140, 800 * 120, 1600), dict(levels=600), full, None))
    return cases


def random_case(rng):
    """a seeded measurement, setting, range and state"""
    full = int(rng.integers(0, 2))
    kind = int(rng.integers(0, 4))
    hist = np.zeros(256, np.int64)
    if kind == 0:
        hist[:] = rng.integers(0, 5000, 256)
    elif kind == 1:
        a, b = sorted(int(v) for v in rng.integers(0, 256, 2))
        hist[a:b + 1] = rng.integers(0, 300, b + 1 - a)
    elif kind == 2:
        for v in rng.integers(0, 256, int(rng.integers(1, 5))):
            hist[v] += int(rng.integers(1, 100000))
    else:
        hist[int(rng.integers(0, 256))] = int(rng.integers(1, 1 << 20))
    nc = int(rng.integers(1, 1 << 20))
    n = int(rng.integers(0, nc + 1)) if rng.integers(0, 2) else int(rng.integers(0, nc // 8 + 1))
    su, sv = (int(rng.integers(0, 255 * n + 1)) for _ in range(2))
    a = {k: int(rng.integers(lo, hi + 1)) for k, (lo, hi) in RANGES.items()}
    prime = bool(rng.integers(0, 4) == 0)
    state = None if prime else (int(rng.integers(0, 65281)), int(rng.integers(0, 65281)), int(rng.integers(-32768, 32768)), int(rng.integers(-32768, 32768)))
    return dict(hist=hist, voters=n, su=su, sv=sv, chroma=nc), a, full, state
