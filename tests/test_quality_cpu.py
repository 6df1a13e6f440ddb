"""tests/qualityref.py -- the numpy restatement of the quality-metrics rule -- against first principles.  No GPU.
The device kernel is held to this restatement bit for bit in tests/test_quality_gpu.py."""
import numpy as np
import pytest

from tests import qualityref as Q


def _coded(n):
    return (n + 15) // 16 * 16


def _surfaces(rng, w, h, fill="noise"):
    """a random NV12 picture of the visible size inside coded-size surfaces whose margin is noise (or zero)"""
    W, H = _coded(w), _coded(h)
    if fill == "noise":
        y, uv = rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, (H // 2, W), dtype=np.uint8)
    else:
        y, uv = np.zeros((H, W), np.uint8), np.zeros((H // 2, W), np.uint8)
    y[:h, :w] = rng.integers(0, 256, (h, w), dtype=np.uint8)
    uv[:h // 2, :w] = rng.integers(0, 256, (h // 2, w), dtype=np.uint8)
    return y, uv


def test_identical_planes_are_perfect():
    rng = np.random.default_rng(1)
    y, uv = _surfaces(rng, 50, 38)
    ints = Q.quality(y, uv, y.copy(), uv.copy(), 50, 38)
    assert ints[:3] == (0, 0, 0)
    q = Q.window_q(y, y, 50, 38)
    assert (q == Q.ONE).all()
    assert ints[3] == Q.ONE * ints[4]
    assert Q.derived(ints, 50, 38) == (100.0, 100.0, 100.0, 1.0)


@pytest.mark.parametrize("w,h", [(16, 16), (50, 38), (64, 48)])
def test_sse_equals_a_plain_sum_in_python_integers(w, h):
    rng = np.random.default_rng(2)
    (ay, auv), (by, buv) = _surfaces(rng, w, h), _surfaces(rng, w, h)
    want = [0, 0, 0]
    for r in range(h):
        for c in range(w):
            want[0] += (int(ay[r, c]) - int(by[r, c])) ** 2
    for r in range(h // 2):
        for c in range(w // 2):
            want[1] += (int(auv[r, 2 * c]) - int(buv[r, 2 * c])) ** 2
            want[2] += (int(auv[r, 2 * c + 1]) - int(buv[r, 2 * c + 1])) ** 2
    assert Q.sse_planes(ay, auv, by, buv, w, h) == want
    psnr = Q.derived(tuple(want) + (Q.ONE, 1), w, h)[:3]
    assert abs(psnr[0] - 10 * np.log10(255.0 ** 2 / (want[0] / (w * h)))) < 1e-9


def _textbook_ssim(a, b):
    """SSIM of one 8x8 window the textbook way, in floats: means, sample variances and covariance (n - 1), and
    (2 mx my + c1)(2 sxy + c2) / ((mx^2 + my^2 + c1)(sx^2 + sy^2 + c2)).  The stabilising constants are those of x264's integer form
    brought to these units: its numerator 2 s1 s2 + C1 is 64^2 (2 mx my + C1 / 64^2), its 2 covar + C2 is 64 * 63 (2 sxy + C2 / (64 * 63))."""
    a, b = a.astype(np.float64).ravel(), b.astype(np.float64).ravel()
    n = a.size
    mx, my = a.mean(), b.mean()
    sx, sy = ((a - mx) ** 2).sum() / (n - 1), ((b - my) ** 2).sum() / (n - 1)
    sxy = ((a - mx) * (b - my)).sum() / (n - 1)
    c1, c2 = Q.C1 / 64.0 ** 2, Q.C2 / (64.0 * 63.0)
    return (2 * mx * my + c1) * (2 * sxy + c2) / ((mx * mx + my * my + c1) * (sx + sy + c2))


@pytest.mark.parametrize("kind", ["random", "close", "flat"])
def test_ssim_agrees_with_the_textbook_formula_per_window(kind):
    rng = np.random.default_rng(3)
    w, h = 52, 36
    a = rng.integers(0, 256, (h, w), dtype=np.uint8)
    if kind == "random":
        b = rng.integers(0, 256, (h, w), dtype=np.uint8)
    elif kind == "close":
        b = np.clip(a.astype(np.int64) + rng.integers(-6, 7, (h, w)), 0, 255).astype(np.uint8)
    else:
        a[:] = 17
        b = np.clip(a.astype(np.int64) + rng.integers(-2, 3, (h, w)), 0, 255).astype(np.uint8)
    q = Q.window_q(a, b, w, h)
    assert q.shape == (h // 4 - 1, w // 4 - 1)
    for by in range(q.shape[0]):
        for bx in range(q.shape[1]):
            want = _textbook_ssim(a[4 * by:4 * by + 8, 4 * bx:4 * bx + 8], b[4 * by:4 * by + 8, 4 * bx:4 * bx + 8])
            assert abs(q[by, bx] / float(Q.ONE) - want) < 2.0 ** -20, (by, bx)


@pytest.mark.parametrize("w,h", [(16, 16), (18, 16), (16, 18), (50, 38), (52, 40), (322, 242)])
def test_window_count_and_left_out_remainder(w, h):
    rng = np.random.default_rng(4)
    (ay, auv), (by, buv) = _surfaces(rng, w, h), _surfaces(rng, w, h)
    ints = Q.quality(ay, auv, by, buv, w, h)
    assert ints[4] == (w // 4 - 1) * (h // 4 - 1)
    # the remainder of two columns / rows belongs to the squared error but not to the SSIM
    cy, dy = ay.copy(), by.copy()
    cy[:, 4 * (w // 4):] ^= 0x55
    cy[4 * (h // 4):, :] ^= 0x55
    other = Q.quality(cy, auv, dy, buv, w, h)
    assert other[3:] == ints[3:]
    assert (other[0] != ints[0]) == (w % 4 != 0 or h % 4 != 0)


@pytest.mark.parametrize("w,h", [(50, 38), (130, 98)])
def test_the_margin_of_the_coded_size_does_not_count(w, h):
    rng = np.random.default_rng(5)
    (ay, auv), (by, buv) = _surfaces(rng, w, h, "zero"), _surfaces(rng, w, h, "zero")
    want = Q.quality(ay, auv, by, buv, w, h)
    for planes in ((ay, auv), (by, buv)):
        for p, rows in zip(planes, (h, h // 2)):
            noise = rng.integers(0, 256, p.shape, dtype=np.uint8)
            p[:, w:] = noise[:, w:]
            p[rows:, :] = noise[rows:, :]
    assert Q.quality(ay, auv, by, buv, w, h) == want
    assert Q.quality(ay[:h, :w], auv[:h // 2, :w], by[:h, :w], buv[:h // 2, :w], w, h) == want


def test_window_terms_stay_below_2_53_for_the_extreme_blocks():
    z, f = np.zeros((16, 16), np.uint8), np.full((16, 16), 255, np.uint8)
    rng = np.random.default_rng(6)
    chk = (rng.integers(0, 2, (16, 16)) * 255).astype(np.uint8)
    for a, b in ((z, f), (f, z), (f, f), (z, z), (chk, 255 - chk), (chk, chk)):
        for t in Q.window_terms(a, b, 16, 16):
            assert (np.abs(t) < 2 ** 53).all()
            assert (t.astype(np.float64).astype(np.int64) == t).all()  # converts to binary64 without rounding
        A, B, C, D = Q.window_terms(a, b, 16, 16)
        assert (C > 0).all() and (D > 0).all()
    # all 0 against all 255: the variances vanish, the means differ as much as they can
    q = Q.window_q(z, f, 16, 16)
    assert (q == int(np.rint(Q.C1 * Q.C2 / ((16320.0 ** 2 + Q.C1) * Q.C2) * Q.ONE))).all()
    assert (Q.window_q(f, f, 16, 16) == Q.ONE).all()
