"""CPU: the colour step's table (mi355enc_yuv_coefficients) against tests/yuvref.py, the accuracy of the integer rule over every input, and the numpy
statements of the 10-bit formats the GPU tests go by."""
import ctypes as C

import numpy as np
import pytest

from tests import yuvref as R

PAIRS8 = [(m, fr) for m in (1, 5, 6, 9) for fr in (0, 1)]
# the 30 (source, destination) pairs over matrix {1, 6, 9} x range that differ
DIFFERING = [(a, b) for a in [(m, fr) for m in (1, 6, 9) for fr in (0, 1)] for b in [(m, fr) for m in (1, 6, 9) for fr in (0, 1)] if a != b]


def test_the_table_equals_the_numpy_table_for_all_pairs(E):
    for im, ifr in PAIRS8:
        for om, ofr in PAIRS8:
            assert list(E.yuv_coefficients(im, ifr, om, ofr)) == R.coefficients(im, ifr, om, ofr), (im, ifr, om, ofr)


def test_the_two_tables_of_the_rule_literally(E):
    assert list(E.yuv_coefficients(6, 0, 1, 0)) == [65536, -7573, -13627, 66758, 7512, 4918, 67196, 16, 16]
    assert list(E.yuv_coefficients(6, 1, 1, 0)) == [56284, -6652, -11971, 58642, 6598, 4321, 59027, 0, 16]
    assert list(E.yuv_coefficients(5, 1, 6, 1)) == [65536, 0, 0, 65536, 0, 0, 65536, 0, 0]  # one matrix under two codes: the identity


def test_bad_codes_are_refused(E):
    L, c = E.load(), (C.c_int32 * 9)()
    for args in ((0, 0, 1, 0), (1, 0, 2, 0), (2, 0, 1, 0), (4, 0, 1, 0), (1, 0, 10, 0), (1, 2, 1, 0), (1, 0, 1, -1), (1, 0, 1, 2)):
        assert L.mi355enc_yuv_coefficients(*args, c) == E.ERR_ARG, args
    assert L.mi355enc_yuv_coefficients(1, 0, 6, 0, None) == E.ERR_ARG
    with pytest.raises(E.EncoderError):
        E.yuv_coefficients(3, 0, 1, 0)


@pytest.fixture(scope="module")
def cube():
    """every (Y, Cb, Cr): Y along axis 0, the 65536 chroma pairs along axis 1"""
    y = np.arange(256, dtype=np.int64).reshape(256, 1)
    cb, cr = (c.reshape(1, 65536) for c in np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij"))
    return y, cb, cr


def test_every_unclipped_output_is_within_051_of_the_double_value(cube):
    assert len(DIFFERING) == 30
    y, cb, cr = cube
    worst = 0.0
    for (im, ifr), (om, ofr) in DIFFERING:
        coef = R.coefficients(im, ifr, om, ofr)
        # every term and every sum of the integer rule fits int32
        cyy, cyb, cyr, cbb, cbr, crb, crr, oy, oy2 = coef
        assert abs(cyy) * 255 + (abs(cyb) + abs(cyr)) * 128 + (oy2 << 16) + (1 << 15) < 2 ** 31
        assert max(abs(cbb) + abs(cbr), abs(crb) + abs(crr)) * 128 + (128 << 16) + (1 << 15) < 2 ** 31
        gy, _, _ = R.unclipped(coef, y, cb, cr)
        ey, _, _ = R.exact(im, ifr, om, ofr, y, cb, cr)
        _, gb, gr = R.unclipped(coef, 0, cb, cr)  # (the chroma outputs do not depend on Y: one plane of the cube is all of it)
        _, eb, er = R.exact(im, ifr, om, ofr, 0, cb, cr)
        for got, want in ((gy, ey), (gb, eb), (gr, er)):
            err = float(np.abs(got - want).max())
            worst = max(worst, err)
            assert err <= 0.51, ((im, ifr), (om, ofr), err)
    print("worst distance from the double value: %.4f" % worst)


def test_grey_stays_grey():
    y = np.arange(256)
    for (im, ifr), (om, ofr) in DIFFERING:
        _, gb, gr = R.unclipped(R.coefficients(im, ifr, om, ofr), y, 128, 128)
        assert np.all(gb == 128) and np.all(gr == 128)
    oy, ouv = R.convert(np.arange(256, dtype=np.uint8).reshape(16, 16), np.full((8, 16), 128, np.uint8), R.coefficients(6, 1, 1, 0))
    assert np.all(ouv == 128) and oy[0, 0] == 16 and oy[15, 15] == 235


def test_convert_keeps_the_border_under_a_mask():
    rng = np.random.default_rng(1)
    y, uv = rng.integers(0, 256, (16, 32), dtype=np.uint8), rng.integers(0, 256, (8, 32), dtype=np.uint8)
    coef = R.coefficients(6, 1, 1, 0)
    mask = R.picture_mask(30, 14, dst=(4, 2, 20, 8), method=0)
    assert mask.shape == (16, 32) and mask[2:10, 4:24].all() and mask.sum() == 20 * 8
    oy, ouv = R.convert(y, uv, coef, mask)
    fy, fuv = R.convert(y, uv, coef)
    assert np.array_equal(oy[2:10, 4:24], fy[2:10, 4:24]) and np.array_equal(ouv[1:5, 4:24], fuv[1:5, 4:24])
    keep = ~mask
    assert np.array_equal(oy[keep], y[keep]) and np.array_equal(ouv[0], uv[0]) and np.array_equal(ouv[:, :4], uv[:, :4])
    # a rectangle that reaches the visible picture's edge takes the margin with it; turned by 90r it lies where the rotation puts it
    m = R.picture_mask(30, 14, dst=(10, 0, 20, 14), method=0)
    assert m[:, 10:].all() and not m[:, :10].any()
    m = R.picture_mask(14, 30, dst=(10, 0, 20, 14), method=1)  # pre-orientation 30 x 14, coded 14 x 30
    assert m.shape == (32, 16) and m[10:, :].all() and not m[:10, :].any()


@pytest.mark.parametrize("w", [16, 18, 322])
def test_v210_packs_and_unpacks(w):
    rng = np.random.default_rng(w)
    h = 4
    y, cb, cr = rng.integers(0, 1024, (h, w)), rng.integers(0, 1024, (h, w // 2)), rng.integers(0, 1024, (h, w // 2))
    for noise in (None, rng):
        plane = R.pack_v210(y, cb, cr, noise)
        assert plane.shape == (h, R.v210_row_bytes(w)) and plane.dtype == np.uint8
        gy, gb, gr = R.unpack_v210(plane, w, h)
        assert np.array_equal(gy, y) and np.array_equal(gb, cb) and np.array_equal(gr, cr)
    # the layout, literally: Cb0 Y0 Cr0 | Y1 Cb1 Y2 | Cr1 Y3 Cb2 | Y4 Cr2 Y5
    words = R.pack_v210(np.array([[1, 2, 3, 4, 5, 6]]), np.array([[11, 12, 13]]), np.array([[21, 22, 23]])).view("<u4")[0]
    assert [[int(x >> s) & 1023 for s in (0, 10, 20)] for x in words] == [[11, 1, 21], [2, 12, 3], [22, 4, 13], [5, 23, 6]]
    assert R.v210_row_bytes(1920) == 5120 and R.v210_row_bytes(322) == 864


def test_the_ten_to_eight_bit_rules_at_their_ends():
    v = np.array([0, 1, 2, 1021, 1022, 1023])
    assert list(R.down8(v)) == [0, 0, 1, 255, 255, 255]
    s = np.array([0, 1, 2] + list(range(2039, 2047)))
    assert list(R.down8_rows(s, 0)) == [0, 0, 0, 255, 255, 255, 255, 255, 255, 255, 255]
    assert list(R.down8_rows(np.array([3, 4, 2035, 2036]), 0)) == [0, 1, 254, 255]
    # through the formats: the ignored bits do not matter, the margin repeats the last sample
    w, h = 18, 2
    y = np.full((h, w), 1023 << 6 | 63, "<u2")
    c = np.full((h // 2, w), 512 << 6, "<u2")
    oy, ouv = R.to_nv12(R.FMT_P010, [y.view(np.uint8), c.view(np.uint8)], w, h)
    assert oy.shape == (16, 32) and np.all(oy == 255) and np.all(ouv == 128)
    y = np.full((h, w), 0xFC00 | 2, "<u2")
    u, v = np.full((h // 2, w // 2), 0xFC00 | 1021, "<u2"), np.full((h // 2, w // 2), 6, "<u2")
    oy, ouv = R.to_nv12(R.FMT_I420_10, [p.view(np.uint8) for p in (y, u, v)], w, h)
    assert np.all(oy == 1) and np.all(ouv[:, 0::2] == 255) and np.all(ouv[:, 1::2] == 2)
    oy, ouv = R.to_nv12(R.FMT_GRAY8, [np.full((h, w), 77, np.uint8)], w, h)
    assert np.all(oy == 77) and np.all(ouv == 128)


def test_the_abi_names_the_formats_and_the_mirror_passes_wide_planes_as_bytes(E):
    assert (E.FMT_P010, E.FMT_I420_10, E.FMT_V210, E.FMT_GRAY8) == (14, 15, 16, 17) == tuple(R.DEEP_FMTS)
    hdr = open(E.__file__.replace("ceracoder_amd/enc.py", "include/mi355enc.h")).read()
    for name, val in (("P010", 14), ("I420_10", 15), ("V210", 16), ("GRAY8", 17)):
        assert "MI355ENC_FMT_%s = %d" % (name, val) in hdr
    arrs, pp, ss = E.Encoder._planes(None, [np.arange(12, dtype="<u2").reshape(3, 4), np.zeros((3, 2), "<u4"), np.ones((3, 5), np.uint8)])
    assert [a.dtype for a in arrs] == [np.uint8] * 3 and [a.shape for a in arrs] == [(3, 8), (3, 8), (3, 5)] and list(ss) == [8, 8, 5]
    assert list(arrs[0][0]) == [0, 0, 1, 0, 2, 0, 3, 0]
