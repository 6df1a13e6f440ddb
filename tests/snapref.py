"""JPEG stills, restated in numpy: the box reduction, the padding to whole MCUs, IJG's accurate integer forward DCT (jfdctint, rows
first) and libjpeg's quantiser, into the block layout tests/jpegref.entropy_decode returns.  Everything is exact integer arithmetic (int64 here: the rule
says no intermediate leaves 32 bits, and test_snapshot_cpu checks that on the extremes)."""
import numpy as np

from tests import jpegref

NATURAL = jpegref.NATURAL
Q_BASE = (jpegref.Q_LUMA, jpegref.Q_CHROMA)  # T.81 Annex K.1, natural order


def tables(quality):
    """uint16 (2, 64): the quantisation tables of a quality, natural order"""
    assert 1 <= quality <= 100
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.stack([np.clip((q.astype(np.int64) * scale + 50) // 100, 1, 255) for q in Q_BASE]).astype(np.uint16)


def reduce_plane(p, s, ow, oh):
    """(sum of the s x s source samples at (s x + i, s y + j), coordinates clamped to the plane, + s^2 / 2) >> 2 log2 s, for x < ow, y < oh"""
    p = np.asarray(p).astype(np.int64)
    h, w = p.shape
    ys = np.minimum(np.arange(oh * s), h - 1)
    xs = np.minimum(np.arange(ow * s), w - 1)
    big = p[np.ix_(ys, xs)]
    sums = big.reshape(oh, s, ow, s).sum(axis=(1, 3))
    return ((sums + (s * s) // 2) >> (2 * (s.bit_length() - 1))).astype(np.uint8)


def reduced_planes(y, uv, s):
    """NV12 planes of the visible picture (h, w), (h / 2, w) -> Y (oh, ow), Cb, Cr (ceil(oh / 2), ceil(ow / 2))"""
    h, w = y.shape
    ow, oh = -(-w // s), -(-h // s)
    cw, ch = -(-ow // 2), -(-oh // 2)
    uv = np.asarray(uv)
    return [reduce_plane(y, s, ow, oh), reduce_plane(uv[:, 0::2], s, cw, ch), reduce_plane(uv[:, 1::2], s, cw, ch)]


def _pass(d, n, col):
    """one 8-point pass of jfdctint along the last axis; col False: the row pass (n = 11), True: the column pass (n = 15)"""
    R = lambda x, k: (x + (1 << (k - 1))) >> k
    d = [d[..., i] for i in range(8)]
    t0, t7, t1, t6, t2, t5, t3, t4 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6], d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o = [None] * 8
    o[0] = R(t10 + t11, 2) if col else (t10 + t11) << 2
    o[4] = R(t10 - t11, 2) if col else (t10 - t11) << 2
    z = (t12 + t13) * 4433
    o[2], o[6] = R(z + t13 * 6270, n), R(z - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    z3, z4 = z5 - z3 * 16069, z5 - z4 * 3196
    parts = [z, t13 * 6270, t12 * 15137, z5, z3, z4, t4 * 2446, z1 * 7373, t5 * 16819, z2 * 20995, t6 * 25172, t7 * 12299]
    o[7] = R(t4 * 2446 - z1 * 7373 + z3, n)
    o[5] = R(t5 * 16819 - z2 * 20995 + z4, n)
    o[3] = R(t6 * 25172 - z2 * 20995 + z3, n)
    o[1] = R(t7 * 12299 - z1 * 7373 + z4, n)
    peak = max(int(np.abs(v).max()) for v in parts + [t4 * 2446 - z1 * 7373, t5 * 16819 - z2 * 20995, t6 * 25172 - z2 * 20995, t7 * 12299 - z1 * 7373])
    return np.stack(o, axis=-1), peak


def fdct(blocks):
    """samples (..., 8, 8) -> (coefficients (..., 8, 8) int64, 8 x the DCT; the largest intermediate magnitude of either pass)"""
    d = np.asarray(blocks).astype(np.int64) - 128
    ws, p1 = _pass(d, 11, False)                                  # rows
    out, p2 = _pass(ws.swapaxes(-1, -2), 15, True)                # columns
    return out.swapaxes(-1, -2), max(p1, p2 + (1 << 14))


def quantise(coef, q):
    """sign(c) ((|c| + 4 q) / (8 q)), integer division, no clamp"""
    q = np.asarray(q).astype(np.int64).reshape(8, 8)
    a = (np.abs(coef) + 4 * q) // (8 * q)
    return np.where(coef < 0, -a, a)


def plane_blocks(p, bw, bh):
    """a plane padded to bh x bw blocks by repeating its last column and row, as (bh, bw, 8, 8)"""
    p = np.asarray(p)
    p = np.pad(p, ((0, bh * 8 - p.shape[0]), (0, bw * 8 - p.shape[1])), mode="edge")
    return p.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)


def plane_coefs(p, bw=None, bh=None):
    """the unquantised coefficients of a plane's blocks (grey picture layout by default: whole 8 x 8 blocks)"""
    h, w = np.asarray(p).shape
    return fdct(plane_blocks(p, bw or -(-w // 8), bh or -(-h // 8)))[0]


def layout(ow, oh):
    mcux, mcuy = -(-ow // 16), -(-oh // 16)
    return [(2 * mcux, 2 * mcuy), (mcux, mcuy), (mcux, mcuy)]


def levels_of_planes(planes, quality):
    """Y, Cb, Cr of a still (already reduced) -> ([int16 (bh, bw, 8, 8)] per component, qt (2, 64), the largest intermediate)"""
    oh, ow = planes[0].shape
    qt = tables(quality)
    out, peak = [], 0
    for c, (bw, bh) in enumerate(layout(ow, oh)):
        co, pk = fdct(plane_blocks(planes[c], bw, bh))
        lv = quantise(co, qt[1 if c else 0])
        assert np.abs(lv).max() <= 32767
        out.append(lv.astype(np.int16))
        peak = max(peak, pk)
    return out, qt, peak


def levels(y, uv, s=1, quality=75):
    """the rule: NV12 planes of the visible picture -> (levels per component, qt (2, 64), (ow, oh))"""
    planes = reduced_planes(y, uv, s)
    lv, qt, _ = levels_of_planes(planes, quality)
    return lv, qt, (planes[0].shape[1], planes[0].shape[0])


def still(y, uv, s=1, quality=75):
    """the file, by tests/jpegref's writer with the typical tables and a JFIF APP0: what mi355enc_snapshot_write must produce byte for byte"""
    lv, qt, (ow, oh) = levels(y, uv, s, quality)
    return write(lv, qt, ow, oh)


def write(lv, qt, ow, oh):
    """the file of section 18 from levels: SOI, JFIF APP0, two DQT, SOF0, four DHT (DC 0, AC 0, DC 1, AC 1), SOS, scan, EOI"""
    seg = jpegref._seg
    out = bytearray(b"\xff\xd8")
    out += seg(0xE0, b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i in range(2):
        out += seg(0xDB, bytes([i]) + bytes(int(v) for v in np.asarray(qt[i]).ravel()[NATURAL]))
    out += seg(0xC0, bytes([8]) + oh.to_bytes(2, "big") + ow.to_bytes(2, "big") + bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for i in range(2):
        for cl in range(2):
            bits, vals = jpegref.STD_TABLES[(cl, i)]
            out += seg(0xC4, bytes([(cl << 4) | i]) + bytes(bits) + bytes(vals))
    out += seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    body = jpegref.encode_coefs(lv, ow, oh, "420", (qt[0], qt[1]))
    scan = body.index(b"\xff\xda")
    scan += 2 + int.from_bytes(body[scan + 2:scan + 4], "big")
    return bytes(out) + body[scan:]


def picture(w, h, kind, seed=1):
    """NV12 planes of a seeded test picture: 'textured', 'noise' (per-sample noise) or 'saturated' (0 / 255 only)"""
    rng = np.random.default_rng(seed * 7919 + w * 31 + h)
    if kind == "textured":
        y, u, v = jpegref.picture(w, h, seed)
        u, v = u[0::2, 0::2], v[0::2, 0::2]
    elif kind == "noise":
        y, u, v = (rng.integers(0, 256, s).astype(np.uint8) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2)))
    else:
        yy, xx = np.mgrid[0:h, 0:w]
        y = (((xx + yy) & 1) * 255).astype(np.uint8)  # a 0 / 255 checkerboard
        y[h // 2:] = (rng.integers(0, 2, (h - h // 2, w)) * 255).astype(np.uint8)
        u, v = ((rng.integers(0, 2, (h // 2, w // 2)) * 255).astype(np.uint8) for _ in range(2))
    uv = np.empty((h // 2, w), np.uint8)
    uv[:, 0::2], uv[:, 1::2] = u, v
    return np.ascontiguousarray(y), uv
