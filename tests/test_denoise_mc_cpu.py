"""The motion-compensated noise filter without a device: the restatement in tests/denoisemcref.py against tests/denoiseref.py where the
two must agree, the key of mi355enc_denoise_motion_key against the restatement's, the properties the search must have -- vectors that stay inside the surface, a
shift found exactly, a shift out of reach let go --, the margins, and the two quality conditions the rule was chosen for."""
import numpy as np
import pytest

from ceracoder_amd import enc as E
from ceracoder_amd import synth
from tests import denoisemcref as M
from tests import denoiseref as D


def noise_pictures(rng, shape):
    return rng.integers(0, 256, shape, dtype=np.uint8), rng.integers(0, 256, (shape[0] // 2, shape[1]), dtype=np.uint8)


def same4(a, b):
    for g, w in zip(a, b):
        assert (g is None) == (w is None)
        assert g is None or (g.dtype == w.dtype and np.array_equal(g, w))


def test_range_0_is_the_step_without_compensation_bit_for_bit():
    rng = np.random.default_rng(2501)
    for vis, shape in (((48, 32), (32, 48)), ((42, 26), (32, 48))):
        y, uv = noise_pictures(rng, shape)
        near = lambda a: np.clip(16 * a.astype(np.int64) + rng.integers(-60, 61, a.shape), 0, 4080).astype(np.uint16)
        for luma, chroma in ((8, 8), (8, 0), (0, 8)):
            huv = near(uv) if chroma else None
            hy = near(y)
            same4(M.step(y, uv, hy, huv, luma, chroma, 0, visible=vis), D.step(y, uv, hy, huv, luma, chroma, visible=vis))
            same4(M.step(y, uv, None, None, luma, chroma, 8, visible=vis), D.step(y, uv, None, None, luma, chroma, visible=vis))  # priming: no search
    pics = [noise_pictures(rng, (32, 48)) for _ in range(3)]
    for a, b in zip(M.chain(pics, [(8, 8)] * 3, [0] * 3), D.chain(pics, [(8, 8)] * 3)):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("rng_", [1, 4, 16])
def test_identity_with_zero_vectors_where_the_input_equals_the_historys_codes(rng_):
    rng = np.random.default_rng(2502)
    y, uv = noise_pictures(rng, (32, 48))
    y[8:16, 8:24] = 77  # (constant blocks: every candidate inside them costs nothing, the rank decides)
    hy, huv = 16 * y.astype(np.uint16), 16 * uv.astype(np.uint16)
    oy, ouv, nhy, nhuv, vec, m = M.step(y, uv, hy, huv, 8, 8, rng_, vectors=True)
    assert not vec.any() and not m.any()
    assert np.array_equal(oy, y) and np.array_equal(ouv, uv) and np.array_equal(nhy, hy) and np.array_equal(nhuv, huv)


def test_the_key_equals_the_restatements():
    rng = np.random.default_rng(2503)
    cases = [(0, 0, 0, 1), (0, 0, 0, 32), (16320, 0, 0, 32), (16320, 16, 16, 32), (16320, -16, -16, 32), (0, 16, -16, 32), (0, -16, 16, 1), (16320, 16, -16, 0)]
    cases += [(int(rng.integers(0, 16321)), int(rng.integers(-16, 17)), int(rng.integers(-16, 17)), int(rng.integers(0, 33))) for _ in range(2000)]
    for cost, dx, dy, s in cases:
        k = E.denoise_motion_key(cost, dx, dy, s)
        assert k == M.key(cost, dx, dy, s) and k < 1 << 31, (cost, dx, dy, s)
    assert M.key(16320, 16, 16, 32) >> 16 == 16320 + 128 * 32 == 20416
    # the rank is unique per vector and orders shorter vectors first
    ranks = {E.denoise_motion_key(0, dx, dy, 0) for dx in range(-16, 17) for dy in range(-16, 17)}
    assert len(ranks) == 1089 and max(ranks) < 1 << 16 and min(ranks) == E.denoise_motion_key(0, 0, 0, 0) == 16 * 33 + 16
    assert E.denoise_motion_key(5, 1, 0, 0) < E.denoise_motion_key(5, 1, 1, 0) < E.denoise_motion_key(5, -2, 1, 0)
    for bad in ((-1, 0, 0, 8), (16321, 0, 0, 8), (0, 17, 0, 8), (0, 0, -17, 8), (0, 0, 0, 33), (0, 0, 0, -1)):
        assert E.denoise_motion_key(*bad) == 0xFFFFFFFF


def test_every_vector_keeps_its_block_inside_a_32x32_surface_at_range_16():
    rng = np.random.default_rng(2504)
    for _ in range(3):
        y, _ = noise_pictures(rng, (32, 32))
        vec, m = M.search(y, rng.integers(0, 4081, (32, 32), dtype=np.uint16), 8, 16)
        Y, X = np.mgrid[0:4, 0:4] * 8
        assert np.all((X + vec[:, :, 0] >= 0) & (X + vec[:, :, 0] <= 24) & (Y + vec[:, :, 1] >= 0) & (Y + vec[:, :, 1] <= 24))
        assert vec.any() and m.max() <= M.MAX_COST


def shifted(rng, H, W, R, a, b):
    """(cur, hist codes): cur(x, y) = hist(x - a, y - b), cut from one random picture"""
    big = rng.integers(0, 256, (H + 2 * R, W + 2 * R), dtype=np.uint8)
    return np.ascontiguousarray(big[R - b:R - b + H, R - a:R - a + W]), np.ascontiguousarray(big[R:R + H, R:R + W])


@pytest.mark.parametrize("r,a,b", [(4, 4, -4), (4, -3, 1), (8, 5, 8), (16, -16, 16), (16, 7, -9), (1, 1, 0)])
def test_a_shift_within_the_range_is_found_exactly(r, a, b):
    rng = np.random.default_rng(2505)
    H, W = 48, 64
    cur, hist = shifted(rng, H, W, 16, a, b)
    cur[16:24, 24:32] = 9  # a constant block: its displaced position holds something else, any vector may win
    vec, m = M.search(cur, 16 * hist.astype(np.uint16), 8, r)
    Y, X = np.mgrid[0:H // 8, 0:W // 8] * 8
    inside = (X - a >= 0) & (X - a <= W - 8) & (Y - b >= 0) & (Y - b <= H - 8)
    inside[2, 3] = False
    assert inside.sum() >= 12
    assert np.all(vec[inside] == (-a, -b)) and not m[inside].any()
    # ... and the filter with it is the identity there: out = c, H' = 16 c
    uv = rng.integers(0, 256, (H // 2, W), dtype=np.uint8)
    oy, _, nhy, _ = M.step(cur, uv, 16 * hist.astype(np.uint16), None, 8, 0, r)
    sel = np.repeat(np.repeat(inside, 8, axis=0), 8, axis=1)
    assert np.array_equal(oy[sel], cur[sel]) and np.array_equal(nhy[sel], 16 * cur[sel].astype(np.uint16))


@pytest.mark.parametrize("r", [1, 4, 8])
def test_a_shift_one_past_the_range_is_let_go(r):
    rng = np.random.default_rng(2506)
    H, W = 48, 64
    cur, hist = shifted(rng, H, W, 16, r + 1, 0)
    uv = rng.integers(0, 256, (H // 2, W), dtype=np.uint8)
    hy = 16 * hist.astype(np.uint16)
    oy, ouv, nhy, nhuv, vec, m = M.step(cur, uv, hy, 16 * uv.astype(np.uint16), 8, 8, r, vectors=True)
    B = D.block_table(8)
    assert not B[np.minimum(255, m >> 4)].any()  # b = 0 in every block
    assert np.array_equal(oy, cur) and np.array_equal(nhy, 16 * cur.astype(np.uint16)) and np.array_equal(ouv, uv)


@pytest.mark.parametrize("vw,vh,W,H", [(42, 26, 48, 32), (64, 44, 64, 48)])
def test_margins_of_the_result_are_replicas_of_the_visible_result(vw, vh, W, H):
    """On a still scene with noise, and on one that moves along the margin (a vector across a margin reads other history rows / columns for the margin's samples of
    a partly visible block than for the last visible one: those need not be replicas)."""
    rng = np.random.default_rng(2507 + vw)
    big = rng.integers(60, 200, (vh + 8, vw + 8), dtype=np.uint8), rng.integers(60, 200, (vh // 2 + 4, vw + 8), dtype=np.uint8)
    for move in ((0, 0), (2, 0)) if vw == W else ((0, 0),):  # (dx, dy) per picture: at 42 x 26 both margins are partly visible, no axis runs along both
        pics = []
        for n in range(3):
            ox, oy_ = move[0] * n, move[1] * n
            y = np.clip(big[0][oy_:oy_ + vh, ox:ox + vw].astype(np.int64) + rng.integers(-6, 7, (vh, vw)), 0, 255).astype(np.uint8)
            uv = np.clip(big[1][oy_ // 2:oy_ // 2 + vh // 2, ox:ox + vw].astype(np.int64) + rng.integers(-6, 7, (vh // 2, vw)), 0, 255).astype(np.uint8)
            pics.append(D.with_margins(y, uv, W, H))
        hy = huv = None
        moved = False
        for n, (y, uv) in enumerate(pics):
            oy, ouv, hy, huv, vec, _ = M.step(y, uv, hy, huv, 8, 8, 4, visible=(vw, vh), vectors=True)
            moved |= vec is not None and bool(vec.any())
            ry, ruv = D.with_margins(oy[:vh, :vw], ouv[:vh // 2, :vw], W, H)
            assert np.array_equal(oy, ry) and np.array_equal(ouv, ruv), (move, n)
            rhy, rhuv = D.with_margins(hy[:vh, :vw], huv[:vh // 2, :vw], W, H)
            assert np.array_equal(hy, rhy) and np.array_equal(huv, rhuv), (move, n)
        assert moved == (move != (0, 0))
        assert not np.array_equal(oy, pics[-1][0]) and not np.array_equal(ouv, pics[-1][1])  # (it did filter)


# ---- the two quality conditions
W_Q, H_Q, N_Q, SIGMA = 640, 368, 8, 3.0


def noisy(clean, seed):
    rng = np.random.default_rng(seed)
    f = lambda p: np.clip(np.rint(p.astype(np.float64) + SIGMA * rng.standard_normal(p.shape)), 0, 255).astype(np.uint8)
    return [(f(y), f(uv)) for y, uv in clean]


def mean_psnr(pics, clean):
    return float(np.mean([D.psnr(p[0], c[0]) for p, c in list(zip(pics, clean))[N_Q - 4:]]))


def test_under_a_pan_the_compensated_filter_gains_where_the_plain_one_loses():
    """synth.s2_frames at 640 x 368 (a pan of (+3, -2) a picture, rectangles that move up to 9 samples) plus seeded sigma-3 noise, strength (8, 0), range 9, 8 pictures;
    PSNR-Y of the last 4 against the clean clip, their mean.  Measured with this restatement: unfiltered 38.55 dB, denoiseref.chain 37.99 dB, compensated 40.23 dB
    (at 960 x 544 over 12 pictures, pictures 4 .. 11: 38.55, 37.89 and 41.37 dB; 40.12 dB at range 4)."""
    clean = list(synth.s2_frames(W_Q, H_Q, N_Q))
    pics = noisy(clean, 2508)
    plain = D.chain(pics, [(8, 0)] * N_Q)
    mc = M.chain(pics, [(8, 0)] * N_Q, [9] * N_Q)
    p_in, p_plain, p_mc = mean_psnr(pics, clean), mean_psnr(plain, clean), mean_psnr(mc, clean)
    print("pan: unfiltered %.2f dB, plain %.2f dB, compensated %.2f dB" % (p_in, p_plain, p_mc))
    assert p_mc > p_in and p_mc > p_plain


def test_on_a_still_gradient_the_search_does_not_lock_onto_the_noise():
    """A still smooth gradient at 640 x 368 plus the same noise, strength (8, 0), range 9, 8 pictures, the last 4 measured: the compensated output is at most 0.5 dB
    below denoiseref.chain's.  Measured with this restatement: plain 44.43 dB, compensated 44.13 dB (0.30 dB below); with lambda = 0 the prototype lost 1.95 dB."""
    yy, xx = np.mgrid[0:H_Q, 0:W_Q]
    y = (40 + 0.25 * xx + 0.2 * yy).astype(np.uint8)
    uv = np.full((H_Q // 2, W_Q), 128, np.uint8)
    clean = [(y, uv)] * N_Q
    pics = noisy(clean, 2508)
    p_plain = mean_psnr(D.chain(pics, [(8, 0)] * N_Q), clean)
    p_mc = mean_psnr(M.chain(pics, [(8, 0)] * N_Q, [9] * N_Q), clean)
    print("still gradient: plain %.2f dB, compensated %.2f dB" % (p_plain, p_mc))
    assert p_mc >= p_plain - 0.5
