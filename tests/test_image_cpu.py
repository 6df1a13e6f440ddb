"""The image layers without a device: the colour of a pixel as the ABI hands it out against the numpy restatement of the rule
(tests/imageref.py), properties of that restatement, which the GPU tests compare the kernels with, the PAM reader, and the argument checks
that need no handle."""
import ctypes as C

import numpy as np
import pytest

from tests import cscref
from tests import imageref as R

CORNERS = [(r, g, b) for r in (0, 255) for g in (0, 255) for b in (0, 255)]


def _pic(w, h, seed=1):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w), dtype=np.uint8)


@pytest.mark.parametrize("matrix,full", cscref.MATRIX_RANGE_PAIRS)
def test_image_pixel_equals_the_rule(E, matrix, full):
    L = E.load()
    coef = cscref.coefficients(matrix, full)
    assert list(E.csc_coefficients(matrix, full)) == coef
    rng = np.random.default_rng(100 * matrix + full)
    rgb = np.concatenate([np.array(CORNERS), rng.integers(0, 256, (100000, 3))])
    ry, rcb, rcr = R.pixel(coef, rgb[:, 0], rgb[:, 1], rgb[:, 2])
    out = (C.c_uint8 * 3)()
    for i, (r, g, b) in enumerate(rgb.tolist()):
        assert L.mi355enc_image_pixel(matrix, full, r, g, b, out) == 0
        assert (out[0], out[1], out[2]) == (ry[i], rcb[i], rcr[i]), (r, g, b)
    # black, white and the mid grey of the range land where the range says
    assert E.image_pixel(matrix, full, 0, 0, 0) == ((0, 128, 128) if full else (16, 128, 128))
    assert E.image_pixel(matrix, full, 255, 255, 255) == ((255, 128, 128) if full else (235, 128, 128))


def test_image_pixel_refuses_bad_arguments(E):
    L = E.load()
    out = (C.c_uint8 * 3)()
    for m in (0, 2, 3, 4, 7, 8, 10, -1, 255):
        assert L.mi355enc_image_pixel(m, 0, 1, 2, 3, out) == E.ERR_ARG
    for rgb in ((256, 0, 0), (0, -1, 0), (0, 0, 1000), (-256, 0, 0)):
        assert L.mi355enc_image_pixel(1, 0, *rgb, out) == E.ERR_ARG
    assert L.mi355enc_image_pixel(1, 2, 0, 0, 0, out) == E.ERR_ARG
    assert L.mi355enc_image_pixel(1, 0, 0, 0, 0, None) == E.ERR_ARG
    with pytest.raises(E.EncoderError, match=r"\(%d\)" % E.ERR_ARG):
        E.image_pixel(2, 0, 0, 0, 0)


# ---- properties of the restatement
COEF = cscref.coefficients(6, 0)


def test_opacity_0_and_alpha_0_are_the_identity():
    y, uv = _pic(64, 48)
    img = R.random_image(np.random.default_rng(2), 37, 21)
    for ly in (R.layer(img, 5, 7, opacity=0), R.layer(img * np.array([1, 1, 1, 0], np.uint8), 5, 7), R.layer(img * np.array([1, 1, 1, 0], np.uint8), -3, -4, opacity=77)):
        by, buv = R.blend(y, uv, [ly], COEF)
        assert np.array_equal(by, y) and np.array_equal(buv, uv)
    # (alpha 1 at opacity 127: a = (127 + 128) >> 8 = 0 as well; at 128 it is 1)
    one = np.full((2, 2, 4), 1, np.uint8)
    assert np.array_equal(R.blend(y, uv, [R.layer(one, 0, 0, opacity=127)], COEF)[0], y)


def test_opaque_pixels_replace_luma_and_a_covered_opaque_quad_gets_the_chroma():
    y, uv = _pic(64, 48)
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (10, 12, 4), dtype=np.uint8)
    img[:, :, 3] = 255
    yi, cbi, cri = R.pixel(COEF, img[:, :, 0], img[:, :, 1], img[:, :, 2])
    by, buv = R.blend(y, uv, [R.layer(img, 6, 4)], COEF)  # even place: every quad under the image is fully covered
    assert np.array_equal(by[4:14, 6:18], yi)
    c = buv.reshape(24, 32, 2)
    quad = lambda m: m[0::2, 0::2] + m[0::2, 1::2] + m[1::2, 0::2] + m[1::2, 1::2]
    assert np.array_equal(c[2:7, 3:9, 0], (255 * quad(cbi) + 510) // 1020) and np.array_equal(c[2:7, 3:9, 1], (255 * quad(cri) + 510) // 1020)
    # one colour over the quad: exactly its Cbi / Cri
    flat = np.empty((2, 2, 4), np.uint8)
    flat[:] = (200, 30, 90, 255)
    fy, fcb, fcr = (int(v) for v in R.pixel(COEF, 200, 30, 90))
    by, buv = R.blend(y, uv, [R.layer(flat, 10, 8)], COEF)
    assert (by[8:10, 10:12] == fy).all() and tuple(buv.reshape(24, 32, 2)[4, 5]) == (fcb, fcr)
    mask = np.ones_like(y, bool)
    mask[8:10, 10:12] = False
    assert np.array_equal(by[mask], y[mask])


def test_one_pixel_at_an_odd_place_touches_one_sample_and_one_site():
    y, uv = _pic(64, 48)
    px = np.array([[[255, 255, 255, 200]]], np.uint8)
    by, buv = R.blend(y, uv, [R.layer(px, 5, 7)], COEF)
    dy, duv = by != y, (buv != uv).reshape(24, 32, 2).any(axis=2)
    assert set(map(tuple, np.argwhere(dy))) <= {(7, 5)} and set(map(tuple, np.argwhere(duv))) <= {(3, 2)}
    a = 200
    assert by[7, 5] == (int(y[7, 5]) * (255 - a) + 235 * a + 127) // 255
    c0 = uv.reshape(24, 32, 2)[3, 2].astype(int)
    assert tuple(buv.reshape(24, 32, 2)[3, 2]) == tuple((c0 * (1020 - a) + 128 * a + 510) // 1020)


def test_a_place_outside_draws_nothing_and_the_edges_clip():
    w, h = 64, 48
    y, uv = _pic(w, h)
    img = R.random_image(np.random.default_rng(4), 37, 21)
    for x, yy in ((w, 0), (0, h), (-37, 0), (0, -21), (16384, 16384), (-16384, -16384)):
        by, buv = R.blend(y, uv, [R.layer(img, x, yy)], COEF)
        assert np.array_equal(by, y) and np.array_equal(buv, uv)
    by, buv = R.blend(y, uv, [R.layer(img, w - 1, h - 1)], COEF)  # one pixel of it is inside
    assert (by != y).sum() <= 1 and np.array_equal(by[:h - 1], y[:h - 1])
    big = R.random_image(np.random.default_rng(5), w + 40, h + 20)
    by, buv = R.blend(y, uv, [R.layer(big, -20, -10)], COEF)
    inner, _ = R.blend(y, uv, [R.layer(big[10:10 + h, 20:20 + w], 0, 0)], COEF)
    assert np.array_equal(by, inner)


def test_two_overlapping_layers_do_not_commute():
    y, uv = _pic(64, 48)
    a = np.empty((8, 8, 4), np.uint8)
    a[:] = (255, 0, 0, 128)
    b = np.empty((8, 8, 4), np.uint8)
    b[:] = (0, 0, 255, 128)
    la, lb = R.layer(a, 10, 10), R.layer(b, 12, 12)
    ab, ba = R.blend(y, uv, [la, lb], COEF), R.blend(y, uv, [lb, la], COEF)
    assert not np.array_equal(ab[0], ba[0]) and not np.array_equal(ab[1], ba[1])
    outside = np.ones_like(y, bool)
    outside[12:18, 12:18] = False  # they differ only where both lie
    assert np.array_equal(ab[0][outside], ba[0][outside])
    # and a list of layers is the layers one after the other
    one = R.blend(*R.blend(y, uv, [la], COEF), [lb], COEF)
    assert np.array_equal(one[0], ab[0]) and np.array_equal(one[1], ab[1])


def test_byte_orders_name_the_same_picture():
    y, uv = _pic(64, 48)
    img = R.random_image(np.random.default_rng(6), 9, 7)
    ref = R.blend(y, uv, [R.layer(img, 3, 5, fmt=R.FMT_RGBA)], COEF)
    for f in R.FMTS:
        got = R.blend(y, uv, [R.layer(R.to_fmt(img, f), 3, 5, fmt=f)], COEF)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
        assert np.array_equal(R.rgba(R.to_fmt(img, f), f), img)


def test_random_image_has_its_transparent_and_opaque_quarters():
    for iw, ih in ((1, 1), (3, 5), (37, 21), (248, 140)):
        al = R.random_image(np.random.default_rng(7), iw, ih)[:, :, 3]
        n = iw * ih
        assert (al == 255).sum() * 4 >= n and ((al == 0).sum() * 4 >= n or n == 1)


# ---- the PAM reader
def test_pam_files_round_trip(E):
    img = R.random_image(np.random.default_rng(8), 13, 6)
    assert np.array_equal(E.load_pam(R.pam(img)), img)
    rgb = E.load_pam(R.pam(img, alpha=False))
    assert np.array_equal(rgb[:, :, :3], img[:, :, :3]) and (rgb[:, :, 3] == 255).all()
    assert E.load_pam(R.pam(img), size_only=True) == (13, 6)
    # header lines in any order, comments, blank lines, trailing bytes
    body = img.tobytes()
    alt = b"P7\n# made by hand\nTUPLTYPE RGB_ALPHA\nMAXVAL 255\n\nDEPTH 4\nHEIGHT 6\nWIDTH  13 \nENDHDR\n" + body + b"trailing"
    assert np.array_equal(E.load_pam(alt), img)
    assert E.load_pam(R.pam(np.zeros((1, 4096, 4), np.uint8)), size_only=True) == (4096, 1)


def test_pam_reader_refuses(E):
    L = E.load()
    img = R.random_image(np.random.default_rng(9), 5, 4)
    good = R.pam(img)
    w, h = C.c_int(0), C.c_int(0)
    out = np.empty(5 * 4 * 4, np.uint8)

    def rc(data, cap=out.nbytes, dst=out):
        buf = np.frombuffer(bytes(data), np.uint8)
        return L.mi355enc_image_load_pam(buf.ctypes.data_as(C.c_void_p) if buf.size else None, buf.size, C.byref(w), C.byref(h),
                                         dst.ctypes.data_as(C.c_void_p) if dst is not None else None, cap)
    assert rc(good) == 0 and (w.value, h.value) == (5, 4)
    bad = {
        "magic": good.replace(b"P7\n", b"P6\n", 1),
        "maxval": good.replace(b"MAXVAL 255", b"MAXVAL 65535"),
        "depth against tuple type": good.replace(b"DEPTH 4", b"DEPTH 3"),
        "tuple type against depth": good.replace(b"RGB_ALPHA", b"RGB"),
        "grey": good.replace(b"RGB_ALPHA", b"GRAYSCALE_ALPHA").replace(b"DEPTH 4", b"DEPTH 2"),
        "no ENDHDR": good.replace(b"ENDHDR\n", b""),
        "truncated": good[:-1],
        "width 4097": R.pam(np.zeros((1, 4097, 4), np.uint8)),
        "width 0": good.replace(b"WIDTH 5", b"WIDTH 0"),
        "no height": good.replace(b"HEIGHT 4\n", b""),
        "width twice": good.replace(b"WIDTH 5\n", b"WIDTH 5\nWIDTH 5\n"),
        "unknown line": good.replace(b"ENDHDR", b"COLOUR 1\nENDHDR"),
        "empty": b"",
    }
    for name, data in bad.items():
        assert rc(data) == E.ERR_ARG, name
    assert rc(good, cap=out.nbytes - 1) == -5  # MI355ENC_ERR_OVERFLOW
    assert rc(good, cap=0, dst=None) == 0  # the size-only call takes no room
    assert L.mi355enc_image_load_pam(None, 10, C.byref(w), C.byref(h), None, 0) == E.ERR_ARG
    with pytest.raises(E.EncoderError, match=r"\(%d\)" % E.ERR_ARG):
        E.load_pam(bad["magic"])


# ---- validation that needs no handle (that a handle accepts the valid and refuses each of these is in tests/test_image_gpu.py)
def test_validation_on_a_null_handle(E):
    L = E.load()
    img = np.zeros((4, 4, 4), np.uint8)
    im = E.image_layer(img, 1, 2, 200, E.FMT_BGRX)
    assert (im.w, im.h, im.stride, im.x, im.y, im.opacity, im.fmt) == (4, 4, 16, 1, 2, 200, E.FMT_BGRX)
    assert L.mi355enc_set_image(None, 0, C.byref(im)) == E.ERR_ARG
    assert L.mi355enc_set_image(None, 0, None) == E.ERR_ARG
    assert L.mi355enc_set_image_place(None, 0, 0, 0, 256) == E.ERR_ARG
    assert L.mi355enc_last_image(None, 0, C.byref(E.ImageInfo())) == E.ERR_ARG
    y = np.zeros(16, np.uint8)
    assert L.mi355enc_stage_image(None, C.byref(im), 1, y.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p)) == E.ERR_ARG
    assert L.mi355enc_debug_image_bytes(None) == 0
    assert L.mi355enc_time_stage(None, E.STAGE_IMAGE, 1, C.byref(C.c_double())) == E.ERR_ARG
    assert E.IMAGE_LAYERS == R.LAYERS == 4 and E.IMAGE_MAX_DIM == R.MAX_DIM == 4096
    assert (E.FMT_BGRX, E.FMT_RGBX, E.FMT_XRGB, E.FMT_XBGR) == R.FMTS
    assert C.sizeof(E.ImageLayer) == 40 and C.sizeof(E.ImageInfo) == 24  # int, pointer (8-aligned), six ints / six 32-bit words
