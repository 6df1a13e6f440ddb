"""Shared helpers for the parity tests."""
import numpy as np

from ceracoder_amd import synth


def pad_planes(y, uv):
    """Replicate the last row/column up to the coded (multiple-of-16) size, as the encoder does."""
    h, w = y.shape
    H, W = (h + 15) // 16 * 16, (w + 15) // 16 * 16
    yp = np.empty((H, W), np.uint8)
    yp[:h, :w] = y
    yp[:h, w:] = y[:, w - 1:w]
    yp[h:, :] = yp[h - 1:h, :]
    up = np.empty((H // 2, W), np.uint8)
    up[:h // 2, :w] = uv
    for x in range(w, W, 2):
        up[:h // 2, x] = uv[:, w - 2]
        up[:h // 2, x + 1] = uv[:, w - 1]
    up[h // 2:, :] = up[h // 2 - 1:h // 2, :]
    return yp, up


def frames(w, h, n, kind="s2"):
    gen = synth.s2_frames(w, h, n) if kind == "s2" else synth.s3_frames(w, h, n)
    return [pad_planes(y, uv) + (y, uv) for y, uv in gen]


def mbinfo_equal(a, b, fields):
    return all(np.array_equal(a[f], b[f]) for f in fields)


def first_diff(a, b):
    d = np.argwhere(np.asarray(a) != np.asarray(b))
    return None if len(d) == 0 else (tuple(d[0]), len(d))


def cut_clip(w, h, n, cut):
    """S2 clip with a hard scene change at picture `cut`: from there on the pictures come from the S3 (noise) generator --
    nothing in the new scene is predictable from the old one, as at a real cut."""
    a = list(synth.s2_frames(w, h, n))
    b = list(synth.s3_frames(w, h, n))
    return [(np.ascontiguousarray(y), np.ascontiguousarray(uv)) for y, uv in (a[:cut] + b[cut:])]


def half_static_clip(w, h, n, static_lines):
    """S2 clip whose top `static_lines` lines never change (a still background above a moving scene): whole deblocking
    bands of the P pictures have no edge to filter."""
    fr = list(synth.s2_frames(w, h, n))
    y0, uv0 = fr[0]
    out = []
    for y, uv in fr:
        y, uv = y.copy(), uv.copy()
        y[:static_lines] = y0[:static_lines]
        uv[:static_lines // 2] = uv0[:static_lines // 2]
        out.append((y, uv))
    return out


# ---- the band deblocker's cut (tests/cutref.py): crafted records, pictures that filter visibly, content that steers the cut

def db_picture(mbw, mbh, seed):
    """A pre-filter picture on which the deblocking filter visibly works: a smooth field with steps of 5..30 levels between 4x4 blocks
    (luma) and 4x4 blocks of either chroma component -- small enough to stay under alpha at most QPs (uniform noise does not: |p0 - q0|
    >= alpha turns most filters off)."""
    g = np.random.Generator(np.random.PCG64(seed))
    H, W = mbh * 16, mbw * 16

    def field(h, w, period, blk):
        yy, xx = np.mgrid[0:h, 0:w]
        base = 120.0 + 45.0 * np.sin(xx / (1.7 * period)) * np.cos(yy / period)
        step = g.integers(5, 31, (h // blk, w // blk)) * g.choice([-1, 1], (h // blk, w // blk)) // 2
        return np.clip(np.rint(base) + np.kron(step, np.ones((blk, blk), np.int64)), 0, 255).astype(np.uint8)
    y = field(H, W, 37.0, 4)
    uv = np.empty((H // 2, W), np.uint8)
    uv[:, 0::2] = field(H // 2, W // 2, 23.0, 4)
    uv[:, 1::2] = field(H // 2, W // 2, 29.0, 4)
    return y, uv


def random_records(mbw, mbh, seed, intra=0.06, coded=0.3, t8=0.3, qp=(10, 51)):
    """Seeded records mixing intra macroblocks, coded luma blocks (and chroma bits, which raise no bS), NZ_T8, vector differences of
    3, 4 and 5 quarter samples and QPs qp[0] .. qp[1]."""
    from ceracoder_amd.enc import MBINFO_DTYPE
    g = np.random.Generator(np.random.PCG64(seed))
    n = mbw * mbh
    r = np.zeros(n, MBINFO_DTYPE)
    r["mb_type"] = np.where(g.random(n) < intra, g.choice([0, 2], n), 1)
    r["qp"] = g.integers(qp[0], qp[1] + 1, n)
    nz = np.where(g.random(n) < coded, g.integers(1, 1 << 16, n) & g.integers(0, 1 << 16, n), 0)
    nz |= g.integers(0, 1 << 11, n) << 16
    r["nzmask"] = nz | np.where(g.random(n) < t8, 1 << 27, 0)
    steps = np.array([0, 0, 0, 3, -3, 4, -4, 5, -5])
    r["mvx"] = 20 + g.choice(steps, n)
    r["mvy"] = -8 + np.where(g.random(n) < 0.3, g.choice(steps, n), 0)
    return r


def free_column(records, mbw, mbh, col, rows=None):
    """Make the left macroblock edge of column `col` filter nothing (bS 0) in `rows` (default: every row): both macroblocks inter,
    no coded luma block beside the edge (with or without the 8x8 transform), the same vector.  In place."""
    r = records.reshape(mbh, mbw)
    rows = range(mbh) if rows is None else rows
    for y in rows:
        for x, clear in ((col - 1, 0xF0F0), (col, 0x0F0F)):
            r[y, x]["mb_type"] = 1
            r[y, x]["nzmask"] = int(r[y, x]["nzmask"]) & ~clear
        r[y, col]["mvx"], r[y, col]["mvy"] = r[y, col - 1]["mvx"], r[y, col - 1]["mvy"]
    return records


def marked_records(mbw, mbh, bands, t8=False, qp=30):
    """Records for hand-computed cut fixtures: all P_L0_16x16 with the zero vector and nothing coded, except per band (bands[b]):
    None -- the band filters nothing; a set of columns -- the band has work (a coded block in its first row's first macroblock, left of
    every cut window) and the left edge of each listed column is busy (a coded 4x4 block at the top left of that macroblock in the band's
    first row: bS 2 on the edge's upper segments, nothing on the macroblock's bottom edge).  Every other column is free."""
    from ceracoder_amd.enc import MBINFO_DTYPE
    r = np.zeros((mbh, mbw), MBINFO_DTYPE)
    r["mb_type"] = 1
    r["qp"] = qp
    if t8:
        r["nzmask"] = 1 << 27
    for b, busy in enumerate(bands):
        if busy is None:
            continue
        for c in [0] + sorted(busy):
            r[4 * b, c]["nzmask"] = int(r[4 * b, c]["nzmask"]) | 1
    return r.reshape(-1)


def _fresh_noise(g, h, w):
    return g.integers(0, 256, (h, w), dtype=np.uint8)


def noise_strip_clip(w, h, n, pattern, seed=0x5EED):
    """Engineered for the cut: a still background (a smooth field) under vertical strips of fresh noise.  pattern(mbw, mbh) -> (mbh, mbw)
    bool, True where a macroblock is noise.  A P picture's still macroblocks cost nothing and filter nothing, so the free columns of a band
    are the edges between two still macroblocks -- the pattern places them where a test wants them (the window's edges)."""
    g = np.random.Generator(np.random.PCG64(seed))
    mbw, mbh = (w + 15) // 16, (h + 15) // 16
    noisy = np.kron(pattern(mbw, mbh), np.ones((16, 16), bool))[:h, :w]
    yy, xx = np.mgrid[0:h, 0:w]
    bg = np.clip(np.rint(110 + 50 * np.sin(xx / 61.0) * np.cos(yy / 47.0)), 16, 235).astype(np.uint8)
    bguv = np.empty((h // 2, w), np.uint8)
    bguv[:, 0::2] = 120
    bguv[:, 1::2] = 134
    out = []
    for _ in range(n):
        y, uv = bg.copy(), bguv.copy()
        y[noisy] = _fresh_noise(g, h, w)[noisy]
        nuv = noisy[::2]
        uv[nuv] = _fresh_noise(g, h // 2, w)[nuv]
        out.append((y, uv))
    return out


def flash_clip(w, h, n, every=3):
    """S2 with a full-range inversion every `every` pictures: P pictures that carry intra macroblocks (the gated launch with the cut)."""
    out = []
    for i, (y, uv) in enumerate(synth.s2_frames(w, h, n)):
        if i % every == every - 1:
            y, uv = 255 - y, 255 - uv
        out.append((np.ascontiguousarray(y), np.ascontiguousarray(uv)))
    return out


def letterbox_clip(w, h, n, bar):
    """S2 between black bars of `bar` lines at the top and at the bottom: idle bands above and below busy ones."""
    out = []
    for y, uv in synth.s2_frames(w, h, n):
        y, uv = y.copy(), uv.copy()
        y[:bar], y[h - bar:] = 16, 16
        uv[:bar // 2], uv[(h - bar) // 2:] = 128, 128
        out.append((y, uv))
    return out


def content_clip(kind, w, h, n):
    """The clips of the cut's content tests, by name."""
    if kind == "s1":
        return [(y, uv) for y, uv in synth.s1_frames(w, h, n)]
    if kind == "s4pan":
        return [(y, uv) for y, uv in synth.s4_frames(w, h, n, pan_after=0)]
    if kind == "s3":
        return [(y, uv) for y, uv in synth.s3_frames(w, h, n)]
    if kind == "flash":
        return flash_clip(w, h, n)
    if kind == "letterbox":
        return letterbox_clip(w, h, n, (h // 4) & ~15)
    if kind == "strips":
        return noise_strip_clip(w, h, n, window_edge_pattern)
    raise ValueError(kind)


def window_edge_pattern(mbw, mbh):
    """Noise everywhere but in two still columns groups whose inner edges are the cut window's first and last column (tests/cutref.py,
    window()), and in a still stretch of rows: by macroblock row, (fractions of the height) the right edge free only, then the left
    only, then both, then the right only, then nothing to do, then both.  Built so that bands choose the window's left edge, its right
    edge (at 1080p bit 60 of the mask: the second word), nothing at all under a right-edge cut, and take no bound from idle bands."""
    from tests.cutref import window
    first, last, _ = window(mbw)
    p = np.ones((mbh, mbw), bool)
    left = slice(max(0, first - 6), first + 1)   # still: columns first-6 .. first, so of the window's columns only `first` is free
    right = slice(last - 1, min(mbw, last + 6))  # still: columns last-1 .. last+5, so of the window's columns only `last` is free
    cuts = [int(round(f * mbh)) for f in (0.18, 0.3, 0.47, 0.59, 0.76)]
    for y in range(mbh):
        seg = sum(y >= c for c in cuts)
        if seg in (0, 3):
            p[y, right] = False
        elif seg == 1:
            p[y, left] = False
        elif seg in (2, 5):
            p[y, left] = p[y, right] = False
        else:
            p[y, :] = False
    return p
