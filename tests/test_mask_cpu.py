"""Privacy masks, host side (no device): mi355enc_mask_apply_host against the numpy rule of tests/maskref.py on seeded regions at
42 x 26 and 70 x 50, every refusal at its edge and one step outside, the element's string form, the blur's division for every sum of every radius, ellipse
membership against the inequality in Python integers, and the margin convention on the reference's output.  All comparisons are ==.  The GPU tests
(tests/test_mask_gpu.py) hold the kernels against the same reference."""
import ctypes as C

import numpy as np
import pytest

from tests import chainref
from tests import maskref as R

COEF = R.BT601_LIMITED


def _seeded(rng, w, h):
    regs = []
    for _ in range(int(rng.integers(0, 9))):
        mode = int(rng.integers(1, 4))
        param = 0 if mode == R.FILL else 2 * int(rng.integers(2, 33)) if mode == R.PIXELATE else int(rng.integers(1, 33))
        regs.append((int(rng.integers(-20, w + 10)), int(rng.integers(-20, h + 10)), int(rng.integers(1, w + 30)), int(rng.integers(1, h + 30)), mode, param,
                     int(rng.integers(0, 2)), int(rng.integers(0, 1 << 24))))
    return regs


def _noise(rng, w, h):
    return rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w), dtype=np.uint8)


@pytest.mark.parametrize("w,h", [(42, 26), (70, 50)])
def test_apply_host_equals_the_reference_over_seeded_regions(E, w, h):
    rng = np.random.default_rng(w * 1000 + h)
    changed = 0
    for i in range(60):
        y, uv = _noise(rng, w, h)
        regs = _seeded(rng, w, h)
        coef = E.csc_coefficients((6, 1)[i & 1], (i >> 1) & 1)
        gy, guv = E.mask_apply_host(regs, y, uv, coef)
        wy, wuv = R.apply(y, uv, regs, coef)
        assert np.array_equal(gy, wy) and np.array_equal(guv, wuv), regs
        changed += not np.array_equal(gy, y)
    assert changed > 40  # (the cases do something)


def test_rule_by_hand(E):
    """cases small enough to write down"""
    assert tuple(E.csc_coefficients(6, 0)) == COEF
    assert E.mask_colour(0x000000, COEF) == R.colour(0x000000, COEF) == (16, 128, 128) and E.mask_colour(0xFFFFFF, COEF) == R.colour(0xFFFFFF, COEF) == (235, 128, 128)
    assert E.mask_colour(0xFF0000, COEF) == R.colour(0xFF0000, COEF) and E.mask_colour(0x0000FF, E.csc_coefficients(1, 1)) == R.colour(0x0000FF, E.csc_coefficients(1, 1))
    y, uv = np.arange(64, dtype=np.uint8).reshape(8, 8) * 3, np.arange(32, dtype=np.uint8).reshape(4, 8) * 5
    # an odd 1 x 1 region at (3, 3) rounds outward to the quad at (2, 2); fill with white
    gy, guv = E.mask_apply_host([(3, 3, 1, 1, R.FILL, 0, 0, 0xFFFFFF)], y, uv, COEF)
    wy, wuv = y.copy(), uv.copy()
    wy[2:4, 2:4] = 235
    wuv[1, 2:4] = 128
    assert np.array_equal(gy, wy) and np.array_equal(guv, wuv)
    # pixelate 4 over the whole 8 x 8: four cells, each its rounded mean
    gy, guv = E.mask_apply_host([(0, 0, 8, 8, R.PIXELATE, 4)], y, uv, COEF)
    for cy in (0, 4):
        for cx in (0, 4):
            s = y[cy:cy + 4, cx:cx + 4].astype(int)
            assert (gy[cy:cy + 4, cx:cx + 4] == (s.sum() + 8) // 16).all()
            for k in range(2):
                c = uv[cy // 2:cy // 2 + 2, cx + k:cx + 4:2].astype(int)
                assert (guv[cy // 2:cy // 2 + 2, cx + k:cx + 4:2] == (c.sum() + 2) // 4).all()
    # blur 1 of a 2 x 2 region: every pass clamps to the region, so each row / column pair becomes its rounded mean twice over
    gy, _ = E.mask_apply_host([(4, 4, 2, 2, R.BLUR, 1)], y, uv, COEF)
    q = y[4:6, 4:6].astype(int)
    for _ in range(2):
        q = np.stack([(2 * q[:, 0] + q[:, 1] + 1) // 3, (q[:, 0] + 2 * q[:, 1] + 1) // 3], 1)
        q = np.stack([(2 * q[0] + q[1] + 1) // 3, (q[0] + 2 * q[1] + 1) // 3], 0)
    assert np.array_equal(gy[4:6, 4:6], q) and np.array_equal(np.delete(gy.reshape(-1), [36, 37, 44, 45]), np.delete(y.reshape(-1), [36, 37, 44, 45]))
    # the lowest index wins, and both compute from the untouched picture
    a, b = (0, 0, 6, 6, R.PIXELATE, 4), (2, 2, 6, 6, R.BLUR, 2)
    gy, guv = E.mask_apply_host([a, b], y, uv, COEF)
    ay, _ = E.mask_apply_host([a], y, uv, COEF)
    by, _ = E.mask_apply_host([b], y, uv, COEF)
    assert np.array_equal(gy[:6, :6], ay[:6, :6]) and np.array_equal(gy[6:8, 2:8], by[6:8, 2:8]) and np.array_equal(gy[2:8, 6:8], by[2:8, 6:8])
    # a region wholly outside, and none at all: the picture's own bytes
    for regs in ([(8, 0, 4, 4, R.FILL, 0)], [(-4, 0, 4, 4, R.FILL, 0)], [(0, 8, 4, 4, R.BLUR, 3)], [(0, -5, 4, 4, R.PIXELATE, 4)], []):
        gy, guv = E.mask_apply_host(regs, y, uv, COEF)
        assert np.array_equal(gy, y) and np.array_equal(guv, uv)


BASE = (3, 5, 9, 7, R.BLUR, 2, 0, 0x204060)
EDGES = [(0, -16384, 16384), (1, -16384, 16384), (2, 1, 16384), (3, 1, 16384), (6, 0, 1), (7, 0, 0xFFFFFF)]


@pytest.mark.parametrize("field,lo,hi", EDGES)
def test_every_field_is_refused_one_step_outside_its_range(E, field, lo, hi):
    for v, ok in ((lo, True), (hi, True), (lo - 1, False), (hi + 1, False)):
        if v < 0 and field == 7:
            continue  # (an unsigned field)
        r = list(BASE)
        r[field] = v
        assert E.mask_check([r]) == (0 if ok else E.ERR_ARG), (field, v)


def test_mode_param_and_count_refusals(E):
    ok = [(R.FILL, 0), (R.PIXELATE, 4), (R.PIXELATE, 64), (R.PIXELATE, 34), (R.BLUR, 1), (R.BLUR, 32)]
    bad = [(0, 0), (4, 1), (-1, 4), (R.FILL, -1), (R.FILL, 1), (R.PIXELATE, 2), (R.PIXELATE, 3), (R.PIXELATE, 5), (R.PIXELATE, 63), (R.PIXELATE, 66), (R.BLUR, 0), (R.BLUR, 33)]
    for want, cases in ((0, ok), (E.ERR_ARG, bad)):
        for mode, param in cases:
            r = list(BASE)
            r[4], r[5] = mode, param
            assert E.mask_check([r]) == want, (mode, param)
    assert E.mask_check([BASE] * 8) == 0 and E.mask_check([]) == 0
    c = E.mask([BASE] * 8)
    c.n = 9
    assert E.mask_check(c) == E.ERR_ARG
    c.n = -1
    assert E.mask_check(c) == E.ERR_ARG
    assert E.load().mi355enc_mask_check(None) == E.ERR_ARG
    # a refused configuration changes no byte
    y, uv = np.full((4, 4), 7, np.uint8), np.full((2, 4), 9, np.uint8)
    with pytest.raises(E.EncoderError):
        E.mask_apply_host([(0, 0, 4, 4, R.BLUR, 33)], y, uv, COEF)
    with pytest.raises(E.EncoderError):
        E.mask_apply_host([], np.zeros((4, 3), np.uint8), np.zeros((2, 3), np.uint8), COEF)  # (an odd width)
    # the handle's entry points refuse a null handle
    L = E.load()
    assert L.mi355enc_set_mask(None, None) == E.ERR_ARG and L.mi355enc_get_mask(None, None, None) == E.ERR_ARG and L.mi355enc_last_mask(None, None, None) == E.ERR_ARG
    assert L.mi355enc_debug_mask_bytes(None) == 0 and L.mi355enc_mask_probe(None, None, None, None) == E.ERR_ARG
    ms = C.c_double(0)
    assert L.mi355enc_time_stage(None, E.STAGE_MASK_CELLS, 1, C.byref(ms)) == E.ERR_ARG and L.mi355enc_time_stage(None, E.STAGE_MASK_BLUR, 1, C.byref(ms)) == E.ERR_ARG
    assert (E.STAGE_MASK_CELLS, E.STAGE_MASK_BLUR) == (38, 39)
    assert L.mi355enc_abi_version() == 4


def test_parser(E):
    regs = [(16, 32, 640, 360, R.BLUR, 16, 1), (-20, 0, 64, 64, R.PIXELATE, 8), (1000, 1000, 1, 1, R.FILL, 0, 0)]
    text = R.to_text(regs)
    assert text == "16,32,640,360,3,16,1;-20,0,64,64,2,8,0;1000,1000,1,1,1,0,0"
    got = E.mask_parse(text, 0x123456).as_list()
    assert got == [R.region(r)[:7] + (0x123456,) for r in regs]
    assert E.mask_parse("16,32,640,360,3,16").as_list() == [(16, 32, 640, 360, 3, 16, 0, 0)]  # (the shape is optional)
    assert E.mask_parse("").as_list() == [] and E.mask_parse(" \t").as_list() == []
    assert E.mask_parse(" 1 , 2 ,3,4, +3 , 6 ").as_list() == [(1, 2, 3, 4, 3, 6, 0, 0)]
    # every truncation is parsed to something the check accepts, or refused with the output untouched
    L = E.load()
    for k in range(len(text) + 1):
        c = E.Mask()
        C.memset(C.byref(c), 0x5A, C.sizeof(c))
        before = bytes(c)
        r = L.mi355enc_mask_parse(text[:k].encode(), 0, C.byref(c))
        assert (r == 0 and E.mask_check(c) == 0) or (r == E.ERR_ARG and bytes(c) == before), (k, r)
    junk = ["x", "1,2,3,4,3", "1,2,3,4,0,4", "1,2,3,4,4,4", "1,2,3,4,2,5", "1,2,3,4,3,33", "1,2,3,4,1,1", "1,2,3,4,3,4,2", "1,2,3,4,3,4,0,7", "1,2,3,4,3,4;", ";1,2,3,4,3,4",
            "1,2,3,4,3,4;;1,2,3,4,3,4", "1,,3,4,3,4", "1,2,0,4,3,4", "1 2,3,4,3,4,0", "1,2,3,4,3,4x", "99999999999999999999,2,3,4,3,4", "1,2,3,4,3,-", "1.5,2,3,4,3,4",
            ";".join(["1,1,1,1,1,0"] * 9)]
    for t in junk:
        with pytest.raises(E.EncoderError):
            E.mask_parse(t)
    assert len(E.mask_parse(";".join(["1,1,1,1,1,0"] * 8)).as_list()) == 8
    with pytest.raises(E.EncoderError):
        E.mask_parse("", 0x1000000)


@pytest.mark.parametrize("r", range(1, 33))
def test_the_division_is_exact_for_every_sum(E, r):
    n = 2 * r + 1
    L = E.load()
    got = [L.mi355enc_mask_mean(s, r) for s in range(255 * n + 1)]
    assert got == [(s + r) // n for s in range(255 * n + 1)]
    assert L.mi355enc_mask_mean(-1, r) == E.ERR_ARG and L.mi355enc_mask_mean(255 * n + 1, r) == E.ERR_ARG


def test_the_division_refuses_radii_outside_its_range(E):
    assert E.mask_mean(0, 0) == E.ERR_ARG and E.mask_mean(0, 33) == E.ERR_ARG


@pytest.mark.parametrize("W2,H2", [(2, 2), (2, 64), (64, 2), (6, 10), (8190, 8190)])
def test_ellipse_membership_is_the_inequality(E, W2, H2):
    nx, ny = W2 // 2, H2 // 2
    if nx * ny <= 4096:
        quads = [(qx, qy) for qy in range(ny) for qx in range(nx)]
    else:  # rows and columns through the middle, at the rim and near 45 degrees, and where the rim crosses every 64th row: the quads either side of it
        rows = sorted(set([0, 1, ny // 2 - 1, ny // 2, ny - 2, ny - 1, 600, 1199, 1200, 2895, 2896]) | set(range(0, ny, 64)))
        quads = [(qx, qy) for qy in rows for qx in range(nx)] + [(qx, qy) for qx in (0, 1, nx // 2, nx - 1, 1199) for qy in range(ny)]
    L = E.load()
    got = [L.mi355enc_mask_ellipse(W2, H2, qx, qy) for qx, qy in quads]
    want = [int(R.ellipse_inside(W2, H2, qx, qy)) for qx, qy in quads]
    assert got == want
    assert sum(want) > 0 and (min(W2, H2) == 2 or sum(want) < len(want))  # (a 2-wide ellipse is its rectangle: dx = 0)
    # the reference's own membership map is that inequality, clipped or not
    if W2 <= 64:
        m = R.membership((0, 0, W2, H2, R.FILL, 0, 1, 0), W2, H2)
        assert m.tolist() == [[R.ellipse_inside(W2, H2, qx, qy) for qx in range(nx)] for qy in range(ny)]
        half = R.membership((-(W2 // 2) & ~1, 0, W2, H2, R.FILL, 0, 1, 0), W2, H2)  # half off the left edge: the same ellipse, cut
        off = (W2 // 2 + 1) // 2 if (W2 // 2) & 1 else W2 // 4
        assert np.array_equal(half[:, :nx - off], m[:, off:])
    assert L.mi355enc_mask_ellipse(W2, H2, nx, 0) == E.ERR_ARG and L.mi355enc_mask_ellipse(W2, H2, 0, -1) == E.ERR_ARG and L.mi355enc_mask_ellipse(W2 + 1, H2, 0, 0) == E.ERR_ARG


def test_margins_are_replicas_with_a_region_over_the_bottom_right_corner():
    rng = np.random.default_rng(5)
    for (w, h), (W, H) in (((42, 26), (48, 32)), ((70, 50), (80, 64))):
        y, uv = _noise(rng, w, h)
        for mode, param, shape in ((R.FILL, 0, 0), (R.PIXELATE, 6, 0), (R.BLUR, 5, 0), (R.BLUR, 3, 1)):
            regs = [(w - 11, h - 9, 40, 40, mode, param, shape, 0x3060C0)]
            cy, cuv = R.coded(y, uv, regs, W, H)
            assert chainref.margins_are_replicas(cy, cuv, w, h)
            vy, vuv = R.apply(y, uv, regs)
            assert np.array_equal(cy[:h, :w], vy) and np.array_equal(cuv[:h // 2, :w], vuv)
            if not shape:  # the corner sample changed, and the whole corner block of the margin is its replica
                assert vy[h - 1, w - 1] != y[h - 1, w - 1] or mode == R.BLUR
                assert (cy[h:, w:] == vy[h - 1, w - 1]).all() and (cuv[h // 2:, w:].reshape(-1, 2) == vuv[h // 2 - 1, w - 2:w]).all()
