"""The temporal noise filter without a device: mi355enc_denoise_tables against the formulas restated in tests/denoiseref.py for every
strength, the argument range at each edge, and the properties the restatement of the step must have -- identity on a still picture, bounded history, a cut
passed through bit for bit, noise actually reduced, margins that are replicas."""
import numpy as np
import pytest

from ceracoder_amd import enc as E
from tests import denoiseref as D


def test_tables_equal_the_formulas_for_every_strength():
    for s in range(1, D.MAX + 1):
        for luma, chroma in ((s, s), (s, 0), (0, s), (s, D.MAX + 1 - s)):
            got = E.denoise_tables(luma=luma, chroma=chroma)
            for g, w in zip(got, D.tables(luma, chroma)):
                assert g.dtype == np.uint8 and np.array_equal(g, w), (luma, chroma)
    # the knees, spelled out for one strength: full weight up to s, none from 3 s on; full weight up to 2 s, none from 6 s on
    B, P, _ = E.denoise_tables(luma=8)
    assert (P[8], P[9], P[23], P[24]) == (224, 210, 14, 0) and (B[16], B[17], B[47], B[48]) == (255, 247, 7, 0)
    assert all(not t.any() for t in E.denoise_tables())


def test_check_refuses_one_past_each_edge():
    for name in ("luma", "chroma"):
        for v, ok in ((-1, False), (0, True), (1, True), (31, True), (32, True), (33, False)):
            assert (E.denoise_check(**{name: v}) == 0) == ok, (name, v)
            if not ok:
                with pytest.raises(E.EncoderError):
                    E.denoise_tables(**{name: v})
    assert E.denoise_check() == 0 and E.denoise().as_dict() == dict(luma=0, chroma=0)
    with pytest.raises(TypeError):
        E.denoise(lumma=3)


def noise_pictures(rng, shape):
    return rng.integers(0, 256, shape, dtype=np.uint8), rng.integers(0, 256, (shape[0] // 2, shape[1]), dtype=np.uint8)


def test_identity_where_the_input_equals_the_history():
    rng = np.random.default_rng(2401)
    y, uv = noise_pictures(rng, (32, 48))
    hy = np.clip(16 * y.astype(np.int64) + rng.integers(-8, 8, y.shape), 0, 4080).astype(np.uint16)  # any H that rounds to the input
    huv = (16 * uv.astype(np.uint16)).astype(np.uint16)
    assert np.array_equal((hy.astype(np.int64) + 8) >> 4, y)
    oy, ouv, nhy, nhuv = D.step(y, uv, 16 * y.astype(np.uint16), huv, 8, 8)
    assert np.array_equal(oy, y) and np.array_equal(ouv, uv) and np.array_equal(nhy, 16 * y.astype(np.uint16)) and np.array_equal(nhuv, huv)
    oy, _, nhy, _ = D.step(y, uv, hy, huv, 8, 8)  # a history within half a code of the input: the output is the input, the history moves towards it, never past it
    assert np.array_equal(oy, y)
    assert np.all(np.abs(nhy.astype(np.int64) - 16 * y.astype(np.int64)) <= np.abs(hy.astype(np.int64) - 16 * y.astype(np.int64)))


def test_history_stays_in_range_for_flips_between_0_and_255():
    for s in (1, 8, 32):
        for c, h in ((0, 4080), (255, 0), (0, 0), (255, 4080)):
            y, uv = np.full((16, 16), c, np.uint8), np.full((8, 16), c, np.uint8)
            hy, huv = np.full((16, 16), h, np.uint16), np.full((8, 16), h, np.uint16)
            hy[:8, :8] = 16 * c  # (one block of each picture matches: b = 255 there, and the rest of it is the flip with b = 0)
            hy[0, 0] = h
            oy, ouv, nhy, nhuv = D.step(y, uv, hy, huv, s, s)
            for a in (nhy, nhuv):
                assert a.dtype == np.uint16 and a.max() <= 4080
            lo, hi = min(16 * c, h), max(16 * c, h)
            assert nhy.min() >= lo and nhy.max() <= hi and np.array_equal(oy[8:], y[8:])


def test_a_cut_passes_through_bit_for_bit():
    rng = np.random.default_rng(2402)
    a, b = noise_pictures(rng, (32, 64)), noise_pictures(rng, (32, 64))
    out = D.chain([a, a, b], [(16, 16)] * 3)
    assert np.array_equal(out[2][0], b[0]) and np.array_equal(out[2][1], b[1])
    out = D.chain([a, b], [(32, 32)] * 2)  # ... at the largest strength too: the mean difference of two noise pictures is about 85 codes, 6 s = 192 quarter codes = 48
    assert np.array_equal(out[1][0], b[0]) and np.array_equal(out[1][1], b[1])


def test_noise_on_a_still_picture_is_reduced():
    """Static content plus seeded Gaussian noise, 12 pictures, 96 x 64: PSNR-Y of the 12th picture against the clean one.  Measured with this restatement:
    sigma 3 at strength 8: input 38.6 dB -> output 47.8 dB (chroma 38.6 -> 47.6); sigma 5 at strength 16: 34.2 dB -> 43.5 dB (chroma 34.2 -> 43.4).
    Recorded, not asserted: the test asks only that the output is strictly closer to the clean picture than the input."""
    for sigma, s in ((3, 8), (5, 16)):
        rng = np.random.default_rng(2403)
        yy, xx = np.mgrid[0:64, 0:96]
        clean = (40 + xx + 0.8 * yy + 30 * ((xx // 16 + yy // 16) & 1)).astype(np.float64)
        cclean = np.full((32, 96), 128.0) + 20 * ((xx[:32] // 8) & 1)
        noisy = lambda p: np.clip(np.rint(p + sigma * rng.standard_normal(p.shape)), 0, 255).astype(np.uint8)
        pics = [(noisy(clean), noisy(cclean)) for _ in range(12)]
        out = D.chain(pics, [(s, s)] * 12)
        gain = [D.psnr(out[-1][k], (clean, cclean)[k]) - D.psnr(pics[-1][k], (clean, cclean)[k]) for k in (0, 1)]
        print("sigma %d strength %d: input %.1f dB, output %.1f dB (chroma %.1f -> %.1f)" % (
            sigma, s, D.psnr(pics[-1][0], clean), D.psnr(out[-1][0], clean), D.psnr(pics[-1][1], cclean), D.psnr(out[-1][1], cclean)))
        assert gain[0] > 0 and gain[1] > 0
        assert np.abs(out[-1][0].astype(np.int64) - clean).sum() < np.abs(pics[-1][0].astype(np.int64) - clean).sum()


@pytest.mark.parametrize("vw,vh,W,H", [(42, 26, 48, 32), (64, 24, 64, 32)])
def test_margins_of_the_result_are_replicas_of_the_visible_result(vw, vh, W, H):
    rng = np.random.default_rng(2404 + vw)
    base = rng.integers(60, 200, (vh, vw), dtype=np.uint8), rng.integers(60, 200, (vh // 2, vw), dtype=np.uint8)
    pics = []
    for _ in range(3):
        y = np.clip(base[0].astype(np.int64) + rng.integers(-6, 7, base[0].shape), 0, 255).astype(np.uint8)
        uv = np.clip(base[1].astype(np.int64) + rng.integers(-6, 7, base[1].shape), 0, 255).astype(np.uint8)
        pics.append(D.with_margins(y, uv, W, H))
    hy = huv = None
    for n, (y, uv) in enumerate(pics):
        oy, ouv, hy, huv = D.step(y, uv, hy, huv, 8, 8, visible=(vw, vh))
        ry, ruv = D.with_margins(oy[:vh, :vw], ouv[:vh // 2, :vw], W, H)
        assert np.array_equal(oy, ry) and np.array_equal(ouv, ruv), n
        rhy, rhuv = D.with_margins(hy[:vh, :vw], huv[:vh // 2, :vw], W, H)
        assert np.array_equal(hy, rhy) and np.array_equal(huv, rhuv), n
    assert not np.array_equal(oy, pics[-1][0]) and not np.array_equal(ouv, pics[-1][1])  # (it did filter)
