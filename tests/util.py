"""Shared helpers for the parity tests."""
import functools

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

@functools.lru_cache(maxsize=8)
def db_picture(mbw, mbh, seed):
    """(Kept per (size, seed), read-only: the crafted-record tests ask for the same few pictures dozens of times, and at 512 rows one costs a second.)  A pre-filter picture on which the deblocking filter visibly works: a smooth field with steps of 5..30 levels between 4x4 blocks
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
    y.setflags(write=False)
    uv.setflags(write=False)
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


# ---- content at the arithmetic limits (tests/test_extremes_cpu.py checks on the oracle that each reaches the branch it was built for;
# ---- tests/test_extremes_gpu.py runs the kernels on it).  Seeded, numpy only; every function returns NV12 planes (y (h, w), uv (h / 2, w)).

def _nv12(u, v):
    uv = np.empty((u.shape[0], 2 * u.shape[1]), np.uint8)
    uv[:, 0::2], uv[:, 1::2] = u, v
    return uv


def _blocks01(g, h, w, blk, share=0.5):
    """(h, w) uint8 of blk x blk blocks, each 0 or 255 (`share` of them 255)"""
    b = (g.random(((h + blk - 1) // blk, (w + blk - 1) // blk)) < share).astype(np.uint8) * np.uint8(255)
    return np.kron(b, np.ones((blk, blk), np.uint8))[:h, :w]


def sat_blocks(w, h, blk, seed):
    """Every blk x blk block (blk 16, 8, 4 or 1) is 0 or 255, in luma and in both chroma components (blocks of blk chroma samples):
    residuals of +-255 over whole blocks (the quantiser's |level| <= 2047 clamp at QP 0), SADs of 65 280, reconstruction at both rails."""
    g = np.random.Generator(np.random.PCG64(seed))
    y = _blocks01(g, h, w, blk)
    return y, _nv12(_blocks01(g, h // 2, w // 2, blk), _blocks01(g, h // 2, w // 2, blk))


def stripes(w, h, period, axis, phase=0):
    """0 / 255 stripes of `period` samples (the first (period + 1) // 2 of every period are 255), axis "v" (vertical stripes), "h" (horizontal) or
    "both" (a checkerboard), moved by `phase` samples along the striped axes; chroma the same pattern on its own grid.  The six-tap filter overshoots
    between two samples of 255 flanked by zeros and undershoots between two zeros flanked by 255; the checkerboard does both in both passes, which
    takes the centre half sample's unrounded intermediates to the two ends of their range."""
    on = (period + 1) // 2

    def plane(ph, pw):
        yy, xx = np.mgrid[0:ph, 0:pw]
        sv, sh = ((xx + phase) % period) < on, ((yy + phase) % period) < on
        m = sv if axis == "v" else sh if axis == "h" else sv ^ sh
        return np.where(m, 255, 0).astype(np.uint8)
    c = plane(h // 2, w // 2)
    return plane(h, w), _nv12(c, c)


def shifted_pair(w, h, dx, dy, seed, half=False):
    """-> ((cur_y, cur_uv), (ref_y, ref_uv)): a full-range texture (uniform noise low-passed once with (1, 2, 1) / 4 in both directions, contrast doubled
    around mid-grey so that it reaches both rails) as the reference, and the same texture displaced as the current picture: cur(x, y) = ref(x + dx, y + dy),
    so the vector of every macroblock whose displaced block lies inside the picture is (dx, dy) whole samples -- with |dx| = |dy| = 16 the corner of the
    +-16 window.  half: the current picture is the rounded average of the displacements (dx, dy) and (dx + sign(dx), dy) -- half a sample further out."""
    g = np.random.Generator(np.random.PCG64(seed))
    m = 40  # margin: the window, the half sample and the filter's support

    def texture(th, tw):
        n = g.integers(0, 256, (th, tw)).astype(np.int64)
        n = (np.roll(n, 1, 1) + 2 * n + np.roll(n, -1, 1) + 2) >> 2
        n = (np.roll(n, 1, 0) + 2 * n + np.roll(n, -1, 0) + 2) >> 2
        return np.clip(2 * (n - 128) + 128, 0, 255)

    def pair(t, ph, pw, mm, sx, sy, hx):
        ref = t[mm:mm + ph, mm:mm + pw]
        cur = t[mm + sy:mm + sy + ph, mm + sx:mm + sx + pw]
        if half:
            cur = (cur + t[mm + sy:mm + sy + ph, mm + sx + hx:mm + sx + hx + pw] + 1) >> 1
        return cur.astype(np.uint8), ref.astype(np.uint8)
    sgn = 1 if dx > 0 else -1
    cy, ry = pair(texture(h + 2 * m, w + 2 * m), h, w, m, dx, dy, sgn)
    tu, tv = texture(h // 2 + m, w // 2 + m), texture(h // 2 + m, w // 2 + m)
    cu, ru = pair(tu, h // 2, w // 2, m // 2, dx // 2, dy // 2, sgn)
    cv, rv = pair(tv, h // 2, w // 2, m // 2, dx // 2, dy // 2, sgn)
    return (cy, _nv12(cu, cv)), (ry, _nv12(ru, rv))


def near_sat_ramps(w, h, seed):
    """Steep planes that run into the rails: every 32 x 32 tile (16 x 16 in chroma) is clip(v0 + sx (x - xc) + sy (y - yc)) with |sx|, |sy| in 3 .. 10 per
    sample, (xc, yc) a point near the tile's centre and v0 within 12 of 0 or of 255 (alternating from tile to tile).  The top row and the left column of the tile's macroblocks are gradients
    that end at a rail, the macroblocks right of and below the tile's first continue their neighbours' plane, and plane prediction (Intra_16x16 and chroma:
    8.3.3.4, 8.3.4.4) extrapolates it below 0 and above 255; the Intra_4x4 / Intra_8x8 modes see the same gradients at the scale of their blocks."""
    g = np.random.Generator(np.random.PCG64(seed))

    def plane(ph, pw, tile):
        ty, tx = (ph + tile - 1) // tile, (pw + tile - 1) // tile
        up = lambda a: np.kron(a, np.ones((tile, tile), np.int64))[:ph, :pw]
        sx = up(g.integers(3, 11, (ty, tx)) * g.choice([-1, 1], (ty, tx)))
        sy = up(g.integers(3, 11, (ty, tx)) * g.choice([-1, 1], (ty, tx)))
        low = (np.add.outer(np.arange(ty), np.arange(tx)) + seed) % 2 == 0  # the rails alternate from tile to tile: both occur in any picture of two tiles
        v0 = up(np.where(low, g.integers(0, 13, (ty, tx)), 255 - g.integers(0, 13, (ty, tx))))
        xc, yc = up(g.integers(tile // 2 - 3, tile // 2 + 4, (ty, tx))), up(g.integers(tile // 2 - 3, tile // 2 + 4, (ty, tx)))
        yy, xx = np.mgrid[0:ph, 0:pw]
        return np.clip(v0 + sx * (xx % tile - xc) + sy * (yy % tile - yc), 0, 255).astype(np.uint8)
    y = plane(h, w, 32)
    return y, _nv12(plane(h // 2, w // 2, 16), plane(h // 2, w // 2, 16))


def db_picture_sat(mbw, mbh, seed):
    """db_picture's twin at the rails: samples of 0 .. 6 in the left half of the picture and of 249 .. 255 in the right half, with steps of 2 .. 9 between
    4x4 blocks of luma and of either chroma component (six of seven towards the rail, clipped to 0 .. 255: blocks that lie on the rail but for a few low
    samples, beside blocks a few levels off it) -- |p0 - q0| stays under alpha from the middle QPs up, and p0 + delta / q0 - delta reach and leave
    0 .. 255 (8.7.2.3: the Clip1 of the bS < 4 filter)."""
    g = np.random.Generator(np.random.PCG64(seed))
    H, W = mbh * 16, mbw * 16

    def field(h, w, blk):
        base = g.integers(0, 7, (h, w))
        step = g.integers(2, 10, (h // blk, w // blk)) * np.where(g.random((h // blk, w // blk)) < 6 / 7, -1, 1)
        v = np.clip(base + np.kron(step, np.ones((blk, blk), np.int64)), 0, 255)
        v[:, w // 2:] = 255 - v[:, w // 2:]
        return v.astype(np.uint8)
    y = field(H, W, 4)
    return y, _nv12(field(H // 2, W // 2, 4), field(H // 2, W // 2, 4))


def sat_clip(w, h, n, seed):
    """n pictures; every macroblock of every picture is drawn from: flat 0, flat 255, flat mid-grey (variance 0: adaptive quantisation's lowest offset),
    a sat_blocks tile of 8 x 8 blocks, a sat_blocks tile of single samples, or -- from the second picture on -- the macroblock of the picture before
    (P_Skip beside saturated neighbours).  Luma and both chroma components alike.  The share of samples at 255 in a single-sample tile is drawn per
    macroblock from 1/2 (the largest variance there is), 1/16 and 1/128, so that adaptive quantisation sees more than its two end offsets."""
    g = np.random.Generator(np.random.PCG64(seed))
    mbw, mbh = (w + 15) // 16, (h + 15) // 16
    y, uv = np.zeros((mbh * 16, mbw * 16), np.uint8), np.zeros((mbh * 8, mbw * 16), np.uint8)
    out = []
    for i in range(n):
        kind = g.integers(0, 6 if i else 5, (mbh, mbw))
        for my in range(mbh):
            for mx in range(mbw):
                k = int(kind[my, mx])
                ys, cs = (slice(my * 16, my * 16 + 16), slice(mx * 16, mx * 16 + 16)), (slice(my * 8, my * 8 + 8), slice(mx * 16, mx * 16 + 16))
                if k < 3:
                    y[ys], uv[cs] = (0, 255, 128)[k], (0, 255, 128)[k]
                elif k < 5:
                    blk, share = (8, 0.5) if k == 3 else (1, (0.5, 0.5, 1 / 16, 1 / 128)[int(g.integers(0, 4))])
                    y[ys] = _blocks01(g, 16, 16, blk, share)
                    uv[cs] = _nv12(_blocks01(g, 8, 8, blk, share), _blocks01(g, 8, 8, blk, share))
        out.append((y[:h, :w].copy(), uv[:h // 2, :w].copy()))
    return out
