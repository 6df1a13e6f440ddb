"""The rule of the spatial noise filter and its noise estimate without a device: the C host functions (dspatial_host.c, through the
mirror) against tests/dspatialref.py bit for bit, and properties of the restatement itself.

Figures of the restatement on its synthetic picture (dspatialref.synthetic: 352 x 288, the left half flat patches, the right half sinusoidal texture, Gaussian
noise; every one of the 1584 blocks votes), recorded here and not asserted as thresholds -- they are properties of one picture:

    sigma   v at the 25th percentile   PSNR against the clean picture: noisy -> filtered with s = 2 sigma
    0        0                          --
    1        7                          47.62 -> 49.77 dB
    2       14                          42.00 -> 44.46 dB
    3       20                          38.55 -> 41.82 dB
    5       34                          34.15 -> 39.40 dB
    8       54                          30.08 -> 36.94 dB

v lies 10 to 17 % below 8 sigma (Immerkaer's estimate in eighths of a code, taken at a low percentile)."""
import ctypes as C

import numpy as np
import pytest

from tests import dspatialref as R

SHAPES = [(16, 16, None, None), (48, 32, None, (42, 26)), (80, 64, (18, 62, 10, 38), None), (80, 64, (18, 80, 10, 64), (70, 50)), (64, 48, None, None)]


def noise(W, H, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, (H // 2, W), dtype=np.uint8)


def test_the_abi_names_the_step(E):
    assert E.STAGE_DENOISE_SPATIAL == 36 and E.STAGE_DENOISE_SPATIAL_AUTO == 37 and E.DENOISE_SPATIAL_MAX == R.MAX == 32
    assert E.denoise_spatial().as_dict() == R.DEFAULT and E.denoise_spatial_check() == 0
    assert E.load().mi355enc_abi_version() == 4
    L, ms = E.load(), C.c_double(0)
    st = E.DenoiseSpatial()
    assert L.mi355enc_set_denoise_spatial(None, C.byref(st)) == E.ERR_ARG and L.mi355enc_get_denoise_spatial(None, C.byref(st)) == E.ERR_ARG
    assert L.mi355enc_last_denoise_spatial(None, None, None) == E.ERR_ARG and L.mi355enc_debug_denoise_spatial_bytes(None) == 0
    assert L.mi355enc_denoise_spatial_probe_stage(None, C.byref(st), None, None, None) == E.ERR_ARG
    assert L.mi355enc_time_stage(None, 36, 1, C.byref(ms)) == E.ERR_ARG and L.mi355enc_time_stage(None, 37, 1, C.byref(ms)) == E.ERR_ARG


def test_the_c_tables_equal_the_restatement(E):
    for s in range(R.MAX + 1):
        weight, filt = E.denoise_spatial_tables(s)
        assert np.array_equal(weight, R.weight_table(s)) and np.array_equal(filt, R.filter_table(s)), s
        if s:
            assert (weight[:s + 1] == 16).all() and (weight[3 * s:] == 0).all() and weight[s + 1] < 16 and (np.diff(weight.astype(int)) <= 0).all()
    assert not E.denoise_spatial_tables(0)[1].any()
    for s in (-1, 33):
        with pytest.raises(E.EncoderError, match=r"\(-1\)"):
            E.denoise_spatial_tables(s)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d%s%s" % (s[0], s[1], "-rect" if s[2] else "", "-vis%dx%d" % s[3] if s[3] else ""))
def test_apply_host_and_measure_host_equal_the_restatement(E, shape):
    W, H, rect, vis = shape
    y, uv = noise(W, H, W + H)
    soft = (y // 4 + 90, uv // 8 + 110)
    for py, puv in ((y, uv), soft):
        for sl, sc in ((1, 1), (8, 8), (32, 32), (8, None), (None, 5), (0, 0), (None, None)):
            got = E.denoise_spatial_apply_host(py, puv, -1 if sl is None else sl, -1 if sc is None else sc, rect, vis)
            want = R.apply(py, puv, sl, sc, rect, vis)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (sl, sc)
        for full in (0, 1):
            got, want = E.denoise_spatial_measure_host(py, rect, vis, full), R.measure(py, rect, vis, full)
            assert np.array_equal(got.pop("hist"), want.pop("hist")) and got == want


CASES = R.decide_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_decide_equals_the_restatement(E, case):
    name, m, a, x = case
    got = E.denoise_spatial_decide(m, a, x, prime=x is None)
    assert got == R.decide(m, a, x, prime=x is None)
    rec = got[0]
    if name == "prime-valid":
        assert rec["valid"] and rec["x"] == 256 * rec["v"] == 256 * 24
    if name in ("prime-invalid", "prime-no-voter"):
        assert not rec["valid"] and rec["x"] == 0 and rec["s_luma"] == 0
    if name == "invalid-while-running":
        assert not rec["valid"] and rec["x"] == 5000
    if name == "speed-256":
        assert rec["x"] == 256 * rec["v"]
    if name == "speed-1":
        assert rec["x"] == 3000 + ((256 * 24 - 3000) >> 8)
    if name == "speed-1-down":
        assert rec["x"] == 9000 + ((256 * 24 - 9000) >> 8) == 8988  # (a floor: -11.2 -> -12)
    if name == "bounds-below-s":
        assert (rec["s_luma"], rec["s_chroma"]) == (3, 1)
    if name == "bounds-above-s":
        assert rec["s_luma"] == rec["s_chroma"] < 31


def test_decide_on_seeded_measurements(E):
    rng = np.random.default_rng(5)
    for _ in range(300):
        bins = rng.integers(0, 256, int(rng.integers(0, 400)))
        m = dict(hist=np.bincount(bins, minlength=256), voters=len(bins), candidates=len(bins) + int(rng.integers(0, 20)) * len(bins) + int(rng.integers(0, 9)))
        a = dict(luma=int(rng.integers(0, 33)), chroma=int(rng.integers(0, 33)), auto_gain=int(rng.integers(250, 8001)), percentile=int(rng.integers(1, 51)),
                 speed=int(rng.integers(1, 257)))
        x = None if rng.integers(0, 4) == 0 else int(rng.integers(0, 65281))
        assert E.denoise_spatial_decide(m, a, x, prime=x is None) == R.decide(m, a, x, prime=x is None)


def test_refusals_for_every_field_out_of_range(E):
    for bad in (dict(luma=-1), dict(luma=33), dict(chroma=-1), dict(chroma=33), dict(auto_gain=-1), dict(auto_gain=1), dict(auto_gain=249), dict(auto_gain=8001),
                dict(percentile=0), dict(percentile=51), dict(speed=0), dict(speed=257)):
        assert E.denoise_spatial_check(dict(dict(luma=4), **bad)) == E.ERR_ARG, bad
    for good in (dict(luma=32, chroma=32), dict(auto_gain=250), dict(auto_gain=8000, percentile=1, speed=1), dict(percentile=50, speed=256), {}):
        assert E.denoise_spatial_check(good) == 0, good
    m = R.decide_cases()[0][1]
    for a, x, prime in ((dict(luma=4), 0, True), (dict(auto_gain=1000), -1, False), (dict(auto_gain=1000), 65281, False), (dict(auto_gain=100), 0, True)):
        with pytest.raises(E.EncoderError, match=r"\(-1\)"):
            E.denoise_spatial_decide(m, a, x, prime=prime)
    y, uv = noise(32, 16, 1)
    for rect, vis in (((1, 32, 0, 16), None), ((0, 34, 0, 16), None), ((16, 32, 0, 16), (14, 16)), (None, (33, 16))):
        with pytest.raises(E.EncoderError, match=r"\(-1\)"):
            E.denoise_spatial_apply_host(y, uv, 4, 4, rect, vis)
        with pytest.raises(E.EncoderError, match=r"\(-1\)"):
            E.denoise_spatial_measure_host(y, rect, vis)
    with pytest.raises(E.EncoderError, match=r"\(-1\)"):
        E.denoise_spatial_apply_host(y, uv, 33, 4)


# ---- properties of the restatement
def test_flat_pictures_and_checkerboards_pass_unchanged():
    y, uv = np.full((32, 48), 97, np.uint8), np.full((16, 48), 131, np.uint8)
    xx, yy = np.meshgrid(np.arange(48), np.arange(32))
    cy, cuv = (((xx + yy) & 1) * 255).astype(np.uint8), ((((xx >> 1) + yy)[:16] & 1) * 255).astype(np.uint8)
    for s in range(R.MAX + 1):
        for py, puv in ((y, uv), (cy, cuv)):  # nothing to average; every difference is 0 or 255 >= 3 s
            oy, ouv = R.apply(py, puv, s, s)
            assert np.array_equal(oy, py) and np.array_equal(ouv, puv), s


def test_strength_32_on_a_ramp_of_slope_1_is_the_binomial_filter():
    xx, yy = np.meshgrid(np.arange(64), np.arange(48))
    y = (40 + xx + yy).astype(np.uint8)  # every difference inside the window is at most 4 <= s: full weight
    uv = np.zeros((24, 64), np.uint8)
    uv[:, 0::2] = (60 + xx[:24, 0::2] // 2 + yy[:24, 0::2])
    uv[:, 1::2] = (200 - xx[:24, 1::2] // 2 - yy[:24, 1::2])
    oy, ouv = R.apply(y, uv, 32, 32)
    P = np.pad(y.astype(np.int64), 2, mode="edge")
    k = np.outer(R.W5, R.W5)
    conv = sum(k[i, j] * P[i:i + 48, j:j + 64] for i in range(5) for j in range(5))
    assert np.array_equal(oy, (conv + 128) >> 8)  # (c + ((sum w (n - c) 16 + 2048) >> 12) = (sum w n + 128) >> 8, the weights summing to 256)
    assert np.array_equal(oy[2:-2, 2:-2], y[2:-2, 2:-2])  # (a plane: the binomial mean of a symmetric window is its centre)
    c = uv.reshape(24, 32, 2).astype(np.int64)
    Pc = np.pad(c, ((1, 1), (1, 1), (0, 0)), mode="edge")
    k3 = np.outer(R.W3, R.W3)
    conv = sum(k3[i, j] * Pc[i:i + 24, j:j + 32] for i in range(3) for j in range(3))
    assert np.array_equal(ouv.reshape(24, 32, 2), (conv + 8) >> 4)


def test_the_output_stays_inside_its_window_and_noise_shrinks():
    """(the window assertion itself sits in dspatialref._plane and runs with every call of apply)"""
    rng = np.random.default_rng(11)
    for s in (1, 3, 8, 20, 32):
        y = np.clip(np.rint(120 + 4 * rng.standard_normal((48, 64))), 0, 255).astype(np.uint8)
        uv = np.clip(np.rint(128 + 4 * rng.standard_normal((24, 64))), 0, 255).astype(np.uint8)
        oy, ouv = R.apply(y, uv, s, s)
        assert oy.astype(int).var() < y.astype(int).var() and ouv.astype(int).var() < uv.astype(int).var()
        wild = noise(64, 48, s)
        R.apply(wild[0], wild[1], s, s)


def test_margins_are_replicas_at_42x26_in_48x32():
    y, uv = noise(48, 32, 4)  # noise in the margin too: it must not be read
    for s in (0, 4, 32):
        oy, ouv = R.apply(y, uv, s, s, visible=(42, 26))
        ry, ruv = R.with_margins(oy[:26, :42], ouv[:13, :42], 48, 32)
        assert np.array_equal(oy, ry) and np.array_equal(ouv, ruv)
        clean = R.apply(*R.with_margins(y[:26, :42], uv[:13, :42], 48, 32), s, s, visible=(42, 26))
        assert np.array_equal(oy, clean[0]) and np.array_equal(ouv, clean[1])
        if s:
            assert not np.array_equal(oy[:26, :42], y[:26, :42])


def test_a_border_keeps_its_bytes_and_is_never_read():
    y, uv = noise(80, 64, 6)
    rect = (18, 62, 10, 38)
    mask = np.zeros((64, 80), bool)
    mask[rect[2]:rect[3], rect[0]:rect[1]] = True
    oy, ouv = R.apply(y, uv, 32, 32, rect)
    assert np.array_equal(oy[~mask], y[~mask]) and np.array_equal(ouv[~mask[0::2]], uv[~mask[0::2]]) and not np.array_equal(oy[mask], y[mask])
    y2, uv2 = np.where(mask, y, 255 - y), np.where(mask[0::2], uv, 255 - uv)
    o2 = R.apply(y2, uv2, 32, 32, rect)
    assert np.array_equal(o2[0][mask], oy[mask]) and np.array_equal(o2[1][mask[0::2]], ouv[mask[0::2]])
    m, m2 = R.measure(y, rect), R.measure(y2, rect)
    assert m["candidates"] == 4 * 2 and np.array_equal(m["hist"], m2["hist"])


def test_the_estimate_is_0_without_noise_and_rises_with_sigma():
    vs = []
    for sigma in (0, 1, 2, 3, 5, 8):
        m = R.measure(R.synthetic(sigma=sigma)[1])
        assert m["voters"] == m["candidates"] == 44 * 36
        vs.append(R.percentile_bin(m["hist"], 25))
    assert vs[0] == 0 and all(a < b for a, b in zip(vs, vs[1:]))


def test_clipped_blocks_do_not_vote():
    y = np.full((16, 32), 120, np.uint8)
    y[:8, :8], y[:8, 8:16], y[8:, :8] = 16, 235, 255
    m = R.measure(y)
    assert m["candidates"] == 8 and m["voters"] == 5 and m["hist"][0] == 5
    assert R.measure(y, full=1)["voters"] == 7  # (full range: the bounds are 15 and 240 -- 16 and 235 are inside, 255 is not)
