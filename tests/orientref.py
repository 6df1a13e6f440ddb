"""The orientation rule of DESIGN.md section 15, restated in numpy: the eight methods of GstVideoOrientationMethod as permutations of samples.
Luma is permuted as a plane of bytes, chroma as an [h/2][w/2] plane of (Cb, Cr) pairs -- a pair is never split or swapped.  No device needed."""
import numpy as np

from tests.util import pad_planes

NAMES = ("identity", "90r", "180", "90l", "horiz", "vert", "ul-lr", "ur-ll")
TRANSPOSING = (1, 3, 6, 7)
GEOMS = [(16, 16), (18, 34), (72, 40), (130, 66), (208, 120), (264, 200)]  # coded (oriented) sizes: tests/test_orient_gpu.py


def plane(a, method):
    """a[h][w] (any trailing axes ride along) -> the oriented plane"""
    if method == 0:
        return a
    if method == 1:
        return np.rot90(a, -1)
    if method == 2:
        return a[::-1, ::-1]
    if method == 3:
        return np.rot90(a, 1)
    if method == 4:
        return a[:, ::-1]
    if method == 5:
        return a[::-1, :]
    if method == 6:
        return np.swapaxes(a, 0, 1)
    if method == 7:
        return np.swapaxes(a[::-1, ::-1], 0, 1)
    raise ValueError(method)


def size(method, w, h):
    return (h, w) if method in TRANSPOSING else (w, h)


def orient(y, uv, method):
    """NV12 (y[h][w], uv[h/2][w] interleaved) -> the oriented NV12 picture, contiguous"""
    h, w = y.shape
    assert uv.shape == (h // 2, w) and w % 2 == 0 and h % 2 == 0
    oy = np.ascontiguousarray(plane(y, method))
    pairs = plane(uv.reshape(h // 2, w // 2, 2), method)
    ouv = np.ascontiguousarray(pairs).reshape(pairs.shape[0], pairs.shape[1] * 2)
    return oy, ouv


def orient_coded(y, uv, method):
    """... with the margin up to whole macroblocks that pad_kernel's rule makes (the last column / row; chroma: the last pair)"""
    return pad_planes(*orient(y, uv, method))


def noise(w, h, seed):
    """per-sample noise, Cb in 0 .. 127 and Cr in 128 .. 255: a swapped pair, a shifted tile or a mirrored word shows"""
    rng = np.random.default_rng(seed)
    y = rng.integers(0, 256, (h, w), dtype=np.uint8)
    uv = np.empty((h // 2, w), np.uint8)
    uv[:, 0::2] = rng.integers(0, 128, (h // 2, w // 2), dtype=np.uint8)
    uv[:, 1::2] = rng.integers(128, 256, (h // 2, w // 2), dtype=np.uint8)
    return y, uv
