"""CPU: colorimetry in the SPS VUI (E.1.1, through a parser of this file's own), the integer RGB -> Y'CbCr matrix the library exports against
tests/cscref.py's derivation and against known answers, and cscref's self-checks."""
import itertools

import numpy as np
import pytest

from ceracoder_amd import enc as E
from oracle import csc as OC
from tests import cscref as R
from tests.spsref import nal_units, sps_of


COLORIMETRIES = [(0, 1, 1, 1), (0, 6, 6, 6), (1, 2, 2, 6), (1, 1, 13, 5), (1, 2, 2, 2), (0, 2, 2, 1), (0, 9, 16, 9), (1, 255, 255, 255), (0, 0, 0, 0), (0, 2, 2, 2)]
GEOMETRIES = [(1920, 1080), (1280, 720), (322, 182), (64, 48), (3840, 2160)]  # 1080 and 322 x 182 are cropped


@pytest.mark.parametrize("t8", [False, True], ids=["baseline", "high"])
@pytest.mark.parametrize("sar", [None, (4, 3), (65535, 1)], ids=["nosar", "sar4x3", "sarbig"])
def test_written_colorimetry_parses_back(t8, sar):
    for (w, h), col in itertools.product(GEOMETRIES, COLORIMETRIES):
        hdr = E.host_write_headers(w, h, 60, 1, t8, colorimetry=col, sar=sar)
        (s,) = sps_of(hdr)
        assert s["colorimetry"] == col, (w, h, col)
        assert s["video_signal_type_present"] == int(col != (0, 2, 2, 2))
        assert s["colour_description_present"] == int(col[1:] != (2, 2, 2))
        if s["video_signal_type_present"]:
            assert s["video_format"] == 5
        assert s["sar"] == sar and s["profile_idc"] == (100 if t8 else 66)
        assert (s["mbw"], s["mbh"]) == ((w + 15) // 16, (h + 15) // 16)
        assert s["crop"] == (None if (w % 16 == 0 and h % 16 == 0) else (0, (-w % 16) // 2, 0, (-h % 16) // 2))
        assert (s["num_units_in_tick"], s["time_scale"], s["fixed_frame_rate"]) == (1, 120, 1)
        assert s["restriction"] == (1, 0, 0, 10, 10, 0, 1)
        assert [t for t, _, _ in nal_units(hdr)] == [7, 8]  # the PPS follows, untouched


def test_unspecified_colorimetry_gives_todays_bytes():
    for (w, h), t8, fps in itertools.product(GEOMETRIES, (False, True), ((60, 1), (30000, 1001))):
        old = E.host_write_headers(w, h, fps[0], fps[1], t8)
        assert E.host_write_headers(w, h, fps[0], fps[1], t8, colorimetry=(0, 2, 2, 2)) == old
        assert E.host_write_headers(w, h, fps[0], fps[1], t8, colorimetry=(0, 2, 2, 2), sar=(0, 0)) == old
        (s,) = sps_of(old)
        assert s["video_signal_type_present"] == 0 and s["sar"] is None
        # with a sample aspect ratio: only the colour fields are new
        a, b = E.host_write_headers(w, h, fps[0], fps[1], t8, sar=(16, 15)), E.host_write_headers(w, h, fps[0], fps[1], t8, colorimetry=(1, 1, 1, 1), sar=(16, 15))
        (sa,), (sb,) = sps_of(a), sps_of(b)
        assert sa["sar"] == sb["sar"] == (16, 15) and sa["colorimetry"] == (0, 2, 2, 2) and sb["colorimetry"] == (1, 1, 1, 1)
        assert {k: v for k, v in sa.items() if not k.startswith(("col", "video"))} == {k: v for k, v in sb.items() if not k.startswith(("col", "video"))}


def test_header_writer_refuses_code_points_out_of_range():
    for col in ((2, 1, 1, 1), (-1, 1, 1, 1), (0, 256, 1, 1), (0, 1, -1, 1), (0, 1, 1, 256)):
        with pytest.raises(RuntimeError):
            E.host_write_headers(640, 480, 30, colorimetry=col)


# ---- the matrix
def test_exported_coefficients_equal_the_derivation():
    for m, fr in R.MATRIX_RANGE_PAIRS:
        c = E.csc_coefficients(m, fr)
        assert list(c) == R.coefficients(m, fr), (m, fr)
        assert c[3] + c[4] + c[5] == 0 and c[6] + c[7] + c[8] == 0  # every grey is exactly 128 / 128
        assert c[0] + c[1] + c[2] == (65536 if fr else R._r(219.0 / 255.0 * 65536.0)) and c[9] == (0 if fr else 16)
        assert c[5] == c[6] > 0 and min(c[0], c[1], c[2]) > 0
    assert list(E.csc_coefficients(5, 0)) == list(E.csc_coefficients(6, 0))
    assert list(E.csc_coefficients(1, 0)) == [11966, 40254, 4064, -6596, -22188, 28784, 28784, -26145, -2639, 16]
    for m in (0, 2, 3, 4, 7, 8, 10, 255, -1):
        with pytest.raises(E.EncoderError):
            E.csc_coefficients(m, 0)
    with pytest.raises(E.EncoderError):
        E.csc_coefficients(1, 2)


def test_known_colours():
    def px(m, fr, r, g, b):
        return tuple(int(v) for v in R.rgb_pixel(list(E.csc_coefficients(m, fr)), r, g, b))
    for m in (1, 6, 9):
        assert px(m, 0, 255, 255, 255) == (235, 128, 128) and px(m, 0, 0, 0, 0) == (16, 128, 128)
        assert px(m, 1, 255, 255, 255) == (255, 128, 128) and px(m, 1, 0, 0, 0) == (0, 128, 128)
        for grey in range(256):
            assert px(m, 0, grey, grey, grey)[1:] == (128, 128) and px(m, 1, grey, grey, grey) == (grey, 128, 128)
    assert [px(1, 0, *c) for c in ((255, 0, 0), (0, 255, 0), (0, 0, 255))] == [(63, 102, 240), (173, 42, 26), (32, 240, 118)]
    assert [px(6, 0, *c) for c in ((255, 0, 0), (0, 255, 0), (0, 0, 255))] == [(81, 90, 240), (145, 54, 34), (41, 240, 110)]


def test_integer_conversion_stays_within_half_a_step_of_the_formula():
    """Bound 0.51: three coefficients rounded at 2^-16 (each off by at most 2^-17, times a component of at most 255: 3 * 255 / 131072 < 0.006; the
    chroma sums carry the same relative error) plus the final rounding to an integer (0.5)."""
    rng = np.random.default_rng(11)
    r, g, b = (rng.integers(0, 256, 120000) for _ in range(3))
    for m, fr in R.MATRIX_RANGE_PAIRS:
        y, cb, cr = R.rgb_pixel(R.coefficients(m, fr), r, g, b)
        ey, ecb, ecr = R.exact(m, fr, r, g, b)
        for got, want in ((y, ey), (cb, ecb), (cr, ecr)):
            err = np.abs(got - np.clip(want, 0, 255)).max()
            assert err <= 0.51, (m, fr, err)


# ---- cscref against itself and against the frozen restatement of the existing formats
SIZES = [(16, 16), (64, 48), (322, 182), (18, 34)]


@pytest.mark.parametrize("w,h", SIZES)
def test_y42b_equals_yuy2_of_the_same_samples(w, h):
    rng = np.random.default_rng(w)
    y, u, v = R.random_planes(R.FMT_Y42B, w, h, rng)
    packed = np.empty((h, 2 * w), np.uint8)
    packed[:, 0::2], packed[:, 1::4], packed[:, 3::4] = y, u, v
    a, b = R.to_nv12(R.FMT_Y42B, [y, u, v], w, h), OC.to_nv12(OC.FMT_YUY2, [packed], w, h)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("w,h", SIZES)
def test_swapped_chroma_formats(w, h):
    rng = np.random.default_rng(h)
    y, u, v = R.random_planes(R.FMT_I420, w, h, rng)
    ref = OC.to_nv12(OC.FMT_I420, [y, u, v], w, h)
    a = R.to_nv12(R.FMT_YV12, [y, v, u], w, h)
    vu = np.empty((h // 2, w), np.uint8)
    vu[:, 0::2], vu[:, 1::2] = v, u
    b = R.to_nv12(R.FMT_NV21, [y, vu], w, h)
    for got in (a, b):
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])


@pytest.mark.parametrize("fmt", R.RGB_FMTS, ids=[R.NAMES[f] for f in R.RGB_FMTS])
def test_constant_colour_gives_constant_planes(fmt):
    w, h = 322, 182
    bpp, ro, go, bo = R.RGB_LAYOUT[fmt]
    for (m, fr), (r, g, b) in itertools.product(R.MATRIX_RANGE_PAIRS, ((200, 30, 90), (0, 255, 7))):
        p = np.full((h, w, bpp), 77, np.uint8)  # (the ignored byte holds something)
        p[:, :, ro], p[:, :, go], p[:, :, bo] = r, g, b
        oy, ouv = R.to_nv12(fmt, [p.reshape(h, bpp * w)], w, h, matrix=m, full_range=fr)
        y, cb, cr = R.rgb_pixel(R.coefficients(m, fr), r, g, b)
        assert oy.shape == (192, 336) and (oy == y).all() and (ouv[:, 0::2] == cb).all() and (ouv[:, 1::2] == cr).all()


def test_y444_of_replicated_chroma_and_the_tap():
    w, h = 64, 48
    rng = np.random.default_rng(3)
    y, u, v = R.random_planes(R.FMT_I420, w, h, rng)
    up = lambda c: np.repeat(np.repeat(c, 2, axis=0), 2, axis=1)
    oy, ouv = R.to_nv12(R.FMT_Y444, [y, up(u), up(v)], w, h)
    assert np.array_equal(oy, y)
    # replicated chroma: the tap sees (left neighbour + 3 x own) twice over
    left = np.concatenate([u[:, :1], u[:, :-1]], axis=1).astype(np.int64)
    assert np.array_equal(ouv[:, 0::2], (2 * left + 6 * u.astype(np.int64) + 4) >> 3)
    one = np.zeros((4, 8), np.uint8)
    one[0, 3] = 80  # an odd column feeds the sites on both sides with weight 1
    assert R.tap8(one).tolist() == [[0, 80, 80, 0], [0, 0, 0, 0]]


def test_matrix_for_unspecified_follows_the_coded_size():
    assert [R.resolve_matrix(2, w, h) for w, h in ((1024, 576), (1026, 576), (1024, 578), (1920, 1080), (640, 480))] == [6, 1, 1, 1, 6]
    assert R.resolve_matrix(9, 640, 480) == 9
