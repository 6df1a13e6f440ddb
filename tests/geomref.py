"""numpy restatement of the input geometry rule, written from the rule's text:

- a geometry: the submitted size in_w x in_h, a crop rectangle (cx, cy, cw, ch) inside it, a destination rectangle (dx, dy, dw, dh) inside the
  pre-orientation target Tw x Th, a border colour (Y, Cb, Cr), default (16, 128, 128);
- valid: all twelve numbers even, every value >= 0, cw, ch, dw, dh >= 2, both rectangles inside their pictures, in_w, in_h <= 8192, per axis
  crop <= 8 dst and dst <= 8 crop;
- tables per axis: s = crop / dst; filter stretch st = max(s, 1) (4:2:2 chroma rows: max(2 s, 1)); taps are the source indices j with
  |j - c| < 2 st, weight K((j - c) / st) with the Catmull-Rom K (a = -0.5), normalised by a sequential sum, quantised q = floor(w 2^14 + 0.5),
  the remainder 2^14 - sum q to the largest q (the lowest index on a tie);
- centres, in samples of the whole submitted plane, i counted from the destination rectangle's first sample:
    luma                        c = cx + (i + 0.5) s - 0.5         (rows: cy)
    chroma columns              c = cx / 2 + ((2 i + 0.5) s - 0.5) / 2
    chroma rows, 4:2:0 input    c = cy / 2 + (i + 0.5) s - 0.5
    chroma rows, 4:2:2 input    c = cy + (2 j + 1) s - 0.5
- a tap index outside the crop rectangle is clamped to the rectangle's edge (what videocrop ! videoscale gives);
- h = (sum q src + 2^7) >> 8 as int16, out = clip((sum q h + 2^19) >> 20, 0, 255);
- inside the destination rectangle the filtered samples, elsewhere in Tw x Th luma Y and chroma pairs (Cb, Cr); the margin up to whole
  macroblocks repeats the last row, column and pair of Tw x Th;
- SAR (cw dh) : (ch dw), reduced (fit into 16 bits by the last continued-fraction convergent that does), exchanged under a transposing
  orientation, absent when 1:1 -- and absent altogether with KEEP_SAR;
- fit_rect(src_w, src_h, Tw, Th): the largest rectangle of the source's aspect ratio inside the target: the constrained axis is filled, the
  other is 2 round(other / 2) (half up; at least 2), capped at the target; dx = ((Tw - dw) / 4) 2, dy likewise.
"""
from fractions import Fraction

import numpy as np

LUMA, CHROMA_V, CHROMA_H, CHROMA_V422 = range(4)
FMT_NV12, FMT_I420, FMT_YUY2, FMT_UYVY = range(4)
BLACK = (16, 128, 128)


def kernel(t):
    t = np.abs(np.asarray(t, np.float64))
    near = (1.5 * t - 2.5) * t * t + 1.0
    far = ((-0.5 * t + 2.5) * t - 4.0) * t + 2.0
    return np.where(t < 1.0, near, np.where(t < 2.0, far, 0.0))


def valid(in_w, in_h, crop, dst, tw, th):
    cx, cy, cw, ch = crop
    dx, dy, dw, dh = dst
    nums = (in_w, in_h, cx, cy, cw, ch, dx, dy, dw, dh, tw, th)
    if any(v % 2 or v < 0 for v in nums) or min(cw, ch, dw, dh) < 2 or in_w > 8192 or in_h > 8192:
        return False
    if cx + cw > in_w or cy + ch > in_h or dx + dw > tw or dy + dh > th:
        return False
    return cw <= 8 * dw and dw <= 8 * cw and ch <= 8 * dh and dh <= 8 * ch


def table(off, crop, dst, kind):
    """-> list of (first source index in the whole plane, [q ...]) per sample of the destination axis; off, crop, dst in luma samples"""
    if off % 2 or crop % 2 or dst % 2 or off < 0 or crop < 2 or dst < 2 or crop > 8 * dst or dst > 8 * crop:
        raise ValueError("not a valid axis: %d + %d -> %d" % (off, crop, dst))
    s = crop / dst
    n = dst if kind == LUMA else dst // 2
    st = max(2.0 * s if kind == CHROMA_V422 else s, 1.0)
    out = []
    for i in range(n):
        if kind == LUMA:
            c = off + (i + 0.5) * s - 0.5
        elif kind == CHROMA_V:
            c = off / 2 + (i + 0.5) * s - 0.5
        elif kind == CHROMA_H:
            c = off / 2 + ((2 * i + 0.5) * s - 0.5) / 2
        else:
            c = off + (2 * i + 1) * s - 0.5
        lo, hi = int(np.floor(c - 2.0 * st)) + 1, int(np.ceil(c + 2.0 * st)) - 1
        j = np.arange(lo, hi + 1)
        w = kernel((j - c) / st)
        w = w / np.cumsum(w)[-1]  # (a sequential sum)
        q = np.floor(w * 16384.0 + 0.5).astype(np.int64)
        q[int(np.argmax(q))] += 16384 - int(q.sum())
        out.append((lo, q))
    return out


def padded(tab):
    """(first (n,), coef (n, taps)) with every entry padded by zero weights to the longest"""
    taps = max(len(q) for _, q in tab)
    first = np.array([f for f, _ in tab], np.int32)
    coef = np.zeros((len(tab), taps), np.int16)
    for i, (_, q) in enumerate(tab):
        coef[i, :len(q)] = q
    return first, coef


def _pass(src, tab, axis, lo, hi, shift, rnd):
    out = []
    for first, q in tab:
        idx = np.clip(np.arange(first, first + len(q)), lo, hi)  # clamped to the crop rectangle's edge
        taken = np.take(src, idx, axis=axis).astype(np.int64)
        qq = np.asarray(q, np.int64).reshape((-1, 1) if axis == 0 else (1, -1))
        out.append(((taken * qq).sum(axis=axis) + rnd) >> shift)
    return np.stack(out, axis=axis)


def resample(src, tab_h, tab_v, x0, x1, y0, y1):
    """one sample plane; the crop covers columns x0 .. x1 and rows y0 .. y1 of it (inclusive)"""
    src = src.astype(np.int64)[y0:y1 + 1]  # (rows outside the crop are never needed: the vertical clamp keeps to y0 .. y1)
    h = _pass(src, tab_h, 1, x0, x1, 8, 1 << 7)
    assert h.min() >= -32768 and h.max() <= 32767
    tv = [(f - y0, q) for f, q in tab_v]
    v = _pass(h.astype(np.int16).astype(np.int64), tv, 0, 0, y1 - y0, 20, 1 << 19)
    return np.clip(v, 0, 255).astype(np.uint8)


def components(fmt, planes, w, h):
    """-> (Y (h, w), U, V) of a picture in `fmt`; chroma (h/2, w/2) for 4:2:0, (h, w/2) for 4:2:2"""
    if fmt == FMT_NV12:
        y, uv = planes[0][:h, :w], planes[1][:h // 2, :w]
        return y, uv[:, 0::2], uv[:, 1::2]
    if fmt == FMT_I420:
        return planes[0][:h, :w], planes[1][:h // 2, :w // 2], planes[2][:h // 2, :w // 2]
    p = planes[0][:h, :2 * w]
    if fmt == FMT_YUY2:
        return p[:, 0::2], p[:, 1::4], p[:, 3::4]
    return p[:, 1::2], p[:, 0::4], p[:, 2::4]


def to_target(fmt, planes, in_w, in_h, crop, dst, tw, th, border=BLACK):
    """(Y (th, tw), U, V (th/2, tw/2)): the pre-orientation target"""
    assert valid(in_w, in_h, crop, dst, tw, th)
    cx, cy, cw, ch = crop
    dx, dy, dw, dh = dst
    y, u, v = components(fmt, planes, in_w, in_h)
    is422 = fmt in (FMT_YUY2, FMT_UYVY)
    ty = resample(y, table(cx, cw, dw, LUMA), table(cy, ch, dh, LUMA), cx, cx + cw - 1, cy, cy + ch - 1)
    tab_ch = table(cx, cw, dw, CHROMA_H)
    if is422:
        tab_cv, r0, r1 = table(cy, ch, dh, CHROMA_V422), cy, cy + ch - 1
    else:
        tab_cv, r0, r1 = table(cy, ch, dh, CHROMA_V), cy // 2, (cy + ch) // 2 - 1
    tu = resample(u, tab_ch, tab_cv, cx // 2, (cx + cw) // 2 - 1, r0, r1)
    tv = resample(v, tab_ch, tab_cv, cx // 2, (cx + cw) // 2 - 1, r0, r1)
    oy = np.full((th, tw), border[0], np.uint8)
    ou = np.full((th // 2, tw // 2), border[1], np.uint8)
    ov = np.full((th // 2, tw // 2), border[2], np.uint8)
    oy[dy:dy + dh, dx:dx + dw] = ty
    ou[dy // 2:(dy + dh) // 2, dx // 2:(dx + dw) // 2] = tu
    ov[dy // 2:(dy + dh) // 2, dx // 2:(dx + dw) // 2] = tv
    return oy, ou, ov


def nv12_surfaces(oy, ou, ov):
    """a visible (Y, U, V) picture -> the coded-size NV12 surfaces (whole macroblocks): the margin repeats the last row, column and pair"""
    th, tw = oy.shape
    W, H = (tw + 15) // 16 * 16, (th + 15) // 16 * 16
    sy = np.zeros((H, W), np.uint8)
    sy[:th, :tw] = oy
    sy[:th, tw:] = oy[:, -1:]
    sy[th:] = sy[th - 1]
    suv = np.zeros((H // 2, W), np.uint8)
    suv[:th // 2, 0:tw:2], suv[:th // 2, 1:tw:2] = ou, ov
    suv[:th // 2, tw::2] = ou[:, -1:]
    suv[:th // 2, tw + 1::2] = ov[:, -1:]
    suv[th // 2:] = suv[th // 2 - 1]
    return sy, suv


def to_nv12(fmt, planes, in_w, in_h, crop, dst, tw, th, border=BLACK):
    """the coded-size NV12 surfaces the geometry launch writes (no orientation)"""
    return nv12_surfaces(*to_target(fmt, planes, in_w, in_h, crop, dst, tw, th, border))


def sar(crop, dst, transposed=False, keep_sar=False):
    """(sar_w, sar_h) of the SPS, or None when the VUI carries no aspect ratio"""
    if keep_sar:
        return None
    f = Fraction(crop[2] * dst[3], crop[3] * dst[2])
    a, b = f.numerator, f.denominator
    p0, q0, p1, q1 = 0, 1, 1, 0  # convergents of a / b
    x, y = a, b
    while y:
        t = x // y
        p2, q2 = t * p1 + p0, t * q1 + q0
        if p2 > 65535 or q2 > 65535:
            break
        p0, q0, p1, q1 = p1, q1, p2, q2
        x, y = y, x % y
    if p1 == q1:
        return None
    return (q1, p1) if transposed else (p1, q1)


def fit_rect(src_w, src_h, tw, th):
    """(dx, dy, dw, dh)"""
    dw, dh = tw, th
    if tw * src_h <= th * src_w:  # the width is the constrained axis: other = tw src_h / src_w
        dh = 2 * ((tw * src_h + src_w) // (2 * src_w))  # 2 round(other / 2), half up
    else:
        dw = 2 * ((th * src_w + src_h) // (2 * src_h))
    dw, dh = max(2, min(dw, tw)), max(2, min(dh, th))
    return ((tw - dw) // 4) * 2, ((th - dh) // 4) * 2, dw, dh
