"""numpy restatement of the downscaling rule, written from the rule's text:

- only downscaling, per axis out <= in <= 8 * out, even sizes;
- separable, horizontal first; Catmull-Rom K(t) (a = -0.5, |t| < 2) stretched by s = in / out: taps are the source indices j with
  |j - c| < 2 s, weight K((j - c) / s), normalised to sum 1, quantised q = floor(w * 2^14 + 0.5); the remainder 2^14 - sum q goes to the
  tap with the largest q (the lowest index on a tie); source indices outside the picture are clamped to the edge;
- centres: luma c = (i + 0.5) s - 0.5; chroma rows (4:2:0) the same on chroma rows; chroma columns cosited with even luma,
  c = ((2 i + 0.5) s - 0.5) / 2; chroma rows from 4:2:2 input: stretch 2 s, c = (2 j + 1) s - 0.5 on the full-height chroma rows;
- h = (sum q src + 2^7) >> 8 as int16, out = clip((sum q h + 2^19) >> 20, 0, 255);
- the coded-size margin repeats the last output row, column and chroma pair.
"""
import numpy as np

LUMA, CHROMA_V, CHROMA_H, CHROMA_V422 = range(4)
FMT_NV12, FMT_I420, FMT_YUY2, FMT_UYVY = range(4)


def kernel(t):
    t = np.abs(np.asarray(t, np.float64))
    near = (1.5 * t - 2.5) * t * t + 1.0
    far = ((-0.5 * t + 2.5) * t - 4.0) * t + 2.0
    return np.where(t < 1.0, near, np.where(t < 2.0, far, 0.0))


def table(n_in, n_out, kind):
    """-> list of (first source index, [q ...]) per output sample of the axis"""
    if n_in % 2 or n_out % 2 or n_out <= 0 or n_out > n_in or n_in > 8 * n_out:
        raise ValueError("not a supported downscale: %d -> %d" % (n_in, n_out))
    s = n_in / n_out
    n = n_out if kind == LUMA else n_out // 2
    st = 2.0 * s if kind == CHROMA_V422 else s
    out = []
    for i in range(n):
        if kind in (LUMA, CHROMA_V):
            c = (i + 0.5) * s - 0.5
        elif kind == CHROMA_H:
            c = ((2 * i + 0.5) * s - 0.5) / 2.0
        else:
            c = (2 * i + 1) * s - 0.5
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


def _pass(src, tab, axis, shift, rnd):
    """one filter pass along `axis` (0 rows, 1 columns) of an int array; clamped source indices"""
    n_src = src.shape[axis]
    out = []
    for first, q in tab:
        idx = np.clip(np.arange(first, first + len(q)), 0, n_src - 1)
        taken = np.take(src, idx, axis=axis).astype(np.int64)
        qq = np.asarray(q, np.int64).reshape((-1, 1) if axis == 0 else (1, -1))
        out.append(((taken * qq).sum(axis=axis) + rnd) >> shift)
    return np.stack(out, axis=axis)


def scale_plane(src, tab_h, tab_v):
    """integer separable filter of one sample plane: horizontal (>> 8, int16), then vertical (>> 20, clip)"""
    h = _pass(src.astype(np.int64), tab_h, 1, 8, 1 << 7)
    assert h.min() >= -32768 and h.max() <= 32767
    v = _pass(h.astype(np.int16).astype(np.int64), tab_v, 0, 20, 1 << 19)
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


def to_nv12(fmt, planes, in_w, in_h, out_w, out_h):
    """the coded-size NV12 surfaces (W = 16 ceil(out_w / 16), H likewise) the scale kernel writes"""
    y, u, v = components(fmt, planes, in_w, in_h)
    ty = scale_plane(y, table(in_w, out_w, LUMA), table(in_h, out_h, LUMA))
    ch = table(in_w, out_w, CHROMA_H)
    cv = table(in_h, out_h, CHROMA_V422 if fmt in (FMT_YUY2, FMT_UYVY) else CHROMA_V)
    tu, tv = scale_plane(u, ch, cv), scale_plane(v, ch, cv)
    W, H = (out_w + 15) // 16 * 16, (out_h + 15) // 16 * 16
    oy = np.zeros((H, W), np.uint8)
    oy[:out_h, :out_w] = ty
    oy[:out_h, out_w:] = ty[:, -1:]
    oy[out_h:] = oy[out_h - 1]
    ouv = np.zeros((H // 2, W), np.uint8)
    ouv[:out_h // 2, 0:out_w:2], ouv[:out_h // 2, 1:out_w:2] = tu, tv
    ouv[:out_h // 2, out_w::2] = tu[:, -1:]
    ouv[:out_h // 2, out_w + 1::2] = tv[:, -1:]
    ouv[out_h // 2:] = ouv[out_h // 2 - 1]
    return oy, ouv
