"""The quality-metrics rule (include/mi355enc.h) restated in numpy: int64 and float64 only.

Inputs are NV12 surfaces (luma plane, interleaved chroma plane) of at least the visible size; only the visible width x height
samples count (chroma: width / 2 x height / 2 per component).
  sse[c]   sum of (src - rec)^2 over the visible samples of Y, Cb, Cr.
  SSIM-Y   x264's integer form: 4x4 blocks anchored at (0, 0), bw = width // 4 by bh = height // 4 of them; a window is the
           2x2 group of blocks at every block position ((bw - 1) (bh - 1) windows); per window q = rint(A B / (C D) * 2^30)
           in binary64 from the exact integers A .. D, round-half-even; ssim_sum = sum of q.
"""
import numpy as np

C1 = 416      # x264: (int)(.01 * .01 * 255 * 255 * 64 + .5)
C2 = 235963   # x264: (int)(.03 * .03 * 255 * 255 * 64 * 63 + .5)
ONE = 1 << 30


def sse_planes(src_y, src_uv, rec_y, rec_uv, width, height):
    """-> [sse_y, sse_cb, sse_cr] as Python ints"""
    d = src_y[:height, :width].astype(np.int64) - rec_y[:height, :width].astype(np.int64)
    c = src_uv[:height // 2, :width].astype(np.int64) - rec_uv[:height // 2, :width].astype(np.int64)
    return [int((d * d).sum()), int((c[:, 0::2] ** 2).sum()), int((c[:, 1::2] ** 2).sum())]


def block_sums(a, b, width, height):
    """the four integer sums of every 4x4 block of the visible luma: (bh, bw) int64 arrays s1, s2, ss, s12"""
    bw, bh = width // 4, height // 4
    a = a[:4 * bh, :4 * bw].astype(np.int64).reshape(bh, 4, bw, 4)
    b = b[:4 * bh, :4 * bw].astype(np.int64).reshape(bh, 4, bw, 4)
    s = lambda v: v.sum(axis=(1, 3))
    return s(a), s(b), s(a * a) + s(b * b), s(a * b)


def window_terms(src_y, rec_y, width, height):
    """A, B, C, D of every window: (bh - 1, bw - 1) int64 arrays"""
    w4 = lambda v: v[:-1, :-1] + v[:-1, 1:] + v[1:, :-1] + v[1:, 1:]
    s1, s2, ss, s12 = (w4(v) for v in block_sums(src_y, rec_y, width, height))
    vars_ = 64 * ss - s1 * s1 - s2 * s2
    covar = 64 * s12 - s1 * s2
    return 2 * s1 * s2 + C1, 2 * covar + C2, s1 * s1 + s2 * s2 + C1, vars_ + C2


def window_q(src_y, rec_y, width, height):
    """q of every window, int64"""
    A, B, C, D = (v.astype(np.float64) for v in window_terms(src_y, rec_y, width, height))
    return np.rint((A * B) / (C * D) * float(ONE)).astype(np.int64)


def quality(src_y, src_uv, rec_y, rec_uv, width, height):
    """-> (sse_y, sse_cb, sse_cr, ssim_sum, ssim_windows): the integers of mi355enc_quality_t"""
    q = window_q(src_y, rec_y, width, height)
    return tuple(sse_planes(src_y, src_uv, rec_y, rec_uv, width, height)) + (int(q.sum()), int(q.size))


def derived(ints, width, height, pictures=1):
    """-> (psnr_y, psnr_cb, psnr_cr, ssim) as the getters derive them from the integers"""
    n = [width * height * pictures] + [(width // 2) * (height // 2) * pictures] * 2
    psnr = [100.0 if not e else 10.0 * np.log10(65025.0 * k / e) for e, k in zip(ints[:3], n)]
    return tuple(psnr) + (ints[3] / (ints[4] * float(ONE)),)
