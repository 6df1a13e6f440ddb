"""The 3D colour LUT step without a device: the C statement (ceracoder_amd/csrc/lut3d_host.c) against tests/lut3dref.py bit for bit --
the coefficients, the rule on seeded noise pictures, the .cube parser on the golden file, on generated text and on every refusal -- the rule against the
double-precision model on the four named cubes, the identity on in-gamut pictures, and the table's check at every edge."""
import ctypes as C
import locale
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import lut3dref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "lut3d_small.cube")
# (width, height, picture rectangle x0, x1, y0, y1): the whole picture, a picture of 72 x 80 in surfaces of 80 x 80, a letterbox rectangle inside 208 x 128
SIZES = [(16, 16, None), (80, 80, (0, 72, 0, 80)), (208, 128, (16, 192, 10, 118))]
PAIRS = [(1, 0), (5, 1), (9, 0)]


def noise_picture(w, h, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w), dtype=np.uint8)


def test_exports_are_present(E):
    L = E.load()
    names = [n for n in E.EXPORTS if "lut3d" in n]
    assert len(names) == 12
    for n in names:
        getattr(L, n)
    assert E.STAGE_LUT3D == 35


def test_the_device_entry_points_refuse_a_null_handle_in_front_of_any_hip_call(E, capfd):
    L = E.load()
    buf = np.zeros(64 * 48 * 2, np.uint8)
    p = buf.ctypes.data
    nodes, st, on, gen = E.lut3d_identity(2), E.Lut3d(2, 256), C.c_int(0), C.c_uint(0)
    assert L.mi355enc_set_lut3d(None, C.byref(st), nodes.ctypes.data) == E.ERR_ARG and L.mi355enc_set_lut3d(None, None, None) == E.ERR_ARG
    assert L.mi355enc_get_lut3d(None, C.byref(on), C.byref(st)) == E.ERR_ARG and L.mi355enc_last_lut3d(None, C.byref(st), C.byref(gen)) == E.ERR_ARG
    assert L.mi355enc_debug_lut3d_bytes(None) == 0 and L.mi355enc_debug_lut3d_form(None, 0) == E.ERR_ARG
    for form in (-1, 0, 1):
        assert L.mi355enc_lut3d_probe(None, C.byref(st), nodes.ctypes.data, p, p, form) == E.ERR_ARG
    ms = C.c_double(0)
    assert L.mi355enc_time_stage(None, 35, 1, C.byref(ms)) == E.ERR_ARG and L.mi355enc_time_stage(None, 36, 1, C.byref(ms)) == E.ERR_ARG
    assert "mi355enc:" not in capfd.readouterr().err  # (what HIPCHK prints for a HIP call that failed)


@pytest.mark.parametrize("matrix", [1, 5, 6, 9])
@pytest.mark.parametrize("full", [0, 1])
def test_coefficients_equal_the_references(E, matrix, full):
    got = E.lut3d_coefficients(matrix, full)
    assert got == R.coefficients(matrix, full)
    assert got[18] == (0 if full else 16) and got[0] == got[3] == got[6] and got[1] == got[8] == 0


def test_coefficients_refuse_other_matrices_and_ranges(E):
    out = (C.c_int32 * 19)()
    L = E.load()
    for m in (0, 2, 3, 4, 7, 8, 10, -1):
        assert L.mi355enc_lut3d_coefficients(m, 0, C.byref(out)) == E.ERR_ARG
    assert L.mi355enc_lut3d_coefficients(1, 2, C.byref(out)) == E.ERR_ARG and L.mi355enc_lut3d_coefficients(1, -1, C.byref(out)) == E.ERR_ARG
    assert L.mi355enc_lut3d_coefficients(1, 0, None) == E.ERR_ARG


def test_check_at_every_edge_identity_and_plan(E):
    L = E.load()
    for N in (0, 1, 2, 3, 64, 65, 66, 67):
        ok = R.N_MIN <= N <= R.N_MAX
        nodes = np.zeros(max(N, 1) ** 3, np.uint32)
        assert (E.lut3d_check(nodes, N) == 0) == ok, N
        assert (L.mi355enc_lut3d_identity(N, nodes.ctypes.data) == 0) == ok
        assert (L.mi355enc_lut3d_plan(N) in (E.LUT3D_DIRECT, E.LUT3D_STAGED)) == ok
        if ok:
            assert np.array_equal(nodes, R.identity(N)) and np.array_equal(E.lut3d_identity(N), nodes) and R.check(nodes, N)
    assert L.mi355enc_lut3d_check(None, 2) == E.ERR_ARG and L.mi355enc_lut3d_identity(2, None) == E.ERR_ARG
    nodes = np.full(8, 0x3FFFFFFF, np.uint32)
    assert E.lut3d_check(nodes, 2) == 0
    for k in (0, 7):  # the first and the last node, either of the two top bits
        for bit in (30, 31):
            bad = nodes.copy()
            bad[k] |= np.uint32(1 << bit)
            assert E.lut3d_check(bad, 2) == E.ERR_ARG and not R.check(bad, 2)
    # staged as far as the table fits a compute unit's LDS (34^3 words), direct beyond: profiles/lut3d_price.md
    assert [E.lut3d_plan(N) for N in (2, 17, 33, 34, 35, 65)] == [E.LUT3D_STAGED] * 4 + [E.LUT3D_DIRECT] * 2
    # the identity's fields: round(i 1023 / (N - 1)), ends exact
    for N in (2, 17, 33, 65):
        t = E.lut3d_identity(N)
        assert t[0] == 0 and t[-1] == 0x3FFFFFFF and [int(v) & 1023 for v in t[:N]] == [int(np.floor(i * 1023 / (N - 1) + 0.5)) for i in range(N)]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s[:2])
@pytest.mark.parametrize("N", [2, 3, 17, 33, 65])
def test_apply_host_equals_the_reference_on_noise(E, size, N):
    w, h, rect = size
    y, uv = noise_picture(w, h, 100 * N + w)
    for k, strength in enumerate((1, 128, 255, 256)):
        matrix, full = ((1, 0), (6, 1), (9, 1), (5, 0))[k]
        nodes = R.quantise(R.cube_noise(N, 7 * N + strength))
        wy, wuv = R.apply(nodes, N, strength, matrix, full, y, uv, rect)
        gy, guv = E.lut3d_apply_host(nodes, strength, matrix, full, y, uv, rect)
        assert np.array_equal(gy, wy) and np.array_equal(guv, wuv), (N, strength)
        if rect is not None:  # bytes outside the rectangle are unchanged
            x0, x1, y0, y1 = rect
            my, muv = np.ones(y.shape, bool), np.ones(uv.shape, bool)
            my[y0:y1, x0:x1] = False
            muv[y0 // 2:y1 // 2, x0:x1] = False
            assert np.array_equal(gy[my], y[my]) and np.array_equal(guv[muv], uv[muv])
        assert not np.array_equal(gy, y)
    gy, guv = E.lut3d_apply_host(nodes, 0, 1, 0, y, uv, rect)  # strength 0: the step is off for the picture
    assert np.array_equal(gy, y) and np.array_equal(guv, uv)


def test_apply_host_refuses_what_the_rule_does_not_cover(E):
    y, uv = noise_picture(16, 16, 1)
    nodes = E.lut3d_identity(2)
    for bad in (dict(strength=-1), dict(strength=257), dict(matrix=2), dict(full=2), dict(rect=(1, 16, 0, 16)), dict(rect=(0, 18, 0, 16)), dict(rect=(0, 16, 4, 4)), dict(rect=(0, 16, 0, 18))):
        a = dict(strength=256, matrix=1, full=0, rect=None)
        a.update(bad)
        with pytest.raises(E.EncoderError):
            E.lut3d_apply_host(nodes, a["strength"], a["matrix"], a["full"], y, uv, a["rect"])
    with pytest.raises(E.EncoderError):
        E.lut3d_apply_host(np.full(8, 1 << 30, np.uint32), 256, 1, 0, y, uv)


@pytest.mark.parametrize("name", sorted(R.NAMED))
@pytest.mark.parametrize("N", [2, 17, 33, 65])
def test_the_rule_is_within_one_code_of_the_double_model(E, name, N):
    """64 x 64 uniform-random Y / Cb / Cr, the four named cubes, three matrix / range pairs: every sample of the integer rule (over quantised nodes) lies within
    1 code of the double-precision model (float matrices, float tetrahedral interpolation over unquantised nodes, one rounding at the end)"""
    cube = R.NAMED[name](N)
    nodes = R.quantise(cube)
    for k, (matrix, full) in enumerate(PAIRS):
        y, uv = noise_picture(64, 64, 1000 + 10 * N + k)
        gy, guv = E.lut3d_apply_host(nodes, 256, matrix, full, y, uv)
        my, muv = R.model(cube, N, matrix, full, y, uv)
        dy, dc = np.abs(gy.astype(int) - my).max(), np.abs(guv.astype(int) - muv).max()
        print(name, N, matrix, full, "worst luma", dy, "worst chroma", dc)
        assert dy <= 1 and dc <= 1


@pytest.mark.parametrize("pair", [(1, 0), (1, 1), (6, 0), (6, 1), (9, 0), (9, 1)])
def test_the_identity_returns_in_gamut_pictures_exactly(E, pair):
    """quads of constant colour generated from R'G'B' through the forward matrix: the identity cube of every size gives the input back"""
    matrix, full = pair
    rng = np.random.default_rng(matrix * 2 + full)
    rgb = rng.random((32, 32, 3))
    rgb[0, :8] = [[0, 0, 0], [1, 1, 1], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [0, 1, 1], [1, 0, 1]]
    _, m = R._matrices(matrix, full)
    yuv = np.clip(np.floor(rgb @ np.array(m, np.float64).T + np.array([R._scales(full)[2], 128, 128]) + 0.5), 0, 255).astype(np.uint8)
    y = np.repeat(np.repeat(yuv[..., 0], 2, 0), 2, 1)
    uv = np.ascontiguousarray(yuv[..., 1:]).reshape(32, 64)
    for N in (2, 3, 17, 33, 65):
        gy, guv = E.lut3d_apply_host(E.lut3d_identity(N), 256, matrix, full, y, uv)
        assert np.array_equal(gy, y) and np.array_equal(guv, uv), N


# ------------------------------------------------------------------ the parser
def both_parse(E, text):
    want = R.parse_cube(text)
    got = E.parse_cube(text)
    assert got[1] == want[1] and np.array_equal(got[0], want[0])
    return want


def test_parser_on_the_golden_file(E):
    text = open(GOLDEN, "rb").read()
    assert b"\r\n" in text and b"e-01" in text and b"DOMAIN_MIN" in text and b"TITLE" in text and b"#" in text
    nodes, N = both_parse(E, text)
    assert N == 3 and nodes.size == 27 and E.lut3d_check(nodes, N) == 0
    assert int(nodes[0]) >> 20 == 0 and int(nodes[-1]) >> 20 == 1023  # blue below its domain and above it
    assert both_parse(E, text.replace(b"\r\n", b"\n"))[0].tolist() == nodes.tolist()
    assert both_parse(E, text.decode("ascii").rstrip("\r\n"))[0].tolist() == nodes.tolist()  # no line end behind the last row


@pytest.mark.parametrize("N", [2, 17])
def test_parser_on_generated_text(E, N):
    cube = R.cube_noise(N, N) * 1.5 - 0.25  # below 0 and above 1 as well
    nodes, n = both_parse(E, R.cube_text(cube, N))
    assert n == N and np.abs((nodes & 1023).astype(int) - np.clip(np.round(cube[:, 0] * 1023), 0, 1023)).max() <= 1
    assert np.array_equal(both_parse(E, R.cube_text(R.cube_identity(N), N, eol="\r\n"))[0], R.identity(N))  # (sixteenths are exact in six decimals)


NUMBERS = ["0", "1", "-0", "+1", "0.5", ".5", "5.", "1e0", "1E-3", "12.5e-1", "0.0004887585532746823", "0.00048875855", "0.9995112414467253", "999999", "-999999.999999999",
           "1e5", "0.000001e11", "123456789e-12", "0.123456789987654321", "1e-9", "1e-10", "-1e-9", "9.99999999999e5"]


def test_parser_reads_numbers_as_the_reference_does(E):
    for num in NUMBERS:
        for lo, hi in (("0", "1"), ("-1000", "1000"), ("0.25", "0.75")):
            text = "LUT_3D_SIZE 2\nDOMAIN_MIN %s %s %s\nDOMAIN_MAX %s %s %s\n" % (lo, lo, lo, hi, hi, hi) + ("%s 0 1\n" % num) * 8
            both_parse(E, text)


REFUSED = {
    "lut_1d_size": "LUT_1D_SIZE 2\n" + "0 0 0\n" * 8,
    "size_1": "LUT_3D_SIZE 1\n0 0 0\n",
    "size_66": "LUT_3D_SIZE 66\n",
    "size_fraction": "LUT_3D_SIZE 2.5\n" + "0 0 0\n" * 8,
    "size_twice": "LUT_3D_SIZE 2\nLUT_3D_SIZE 2\n" + "0 0 0\n" * 8,
    "no_size": "0 0 0\n" * 8,
    "too_few_rows": "LUT_3D_SIZE 2\n" + "0 0 0\n" * 7,
    "too_many_rows": "LUT_3D_SIZE 2\n" + "0 0 0\n" * 9,
    "no_rows": "LUT_3D_SIZE 2\n",
    "empty": "",
    "row_of_two": "LUT_3D_SIZE 2\n" + "0 0 0\n" * 7 + "0 0\n",
    "row_of_four": "LUT_3D_SIZE 2\n" + "0 0 0\n" * 7 + "0 0 0 0\n",
    "row_not_a_number": "LUT_3D_SIZE 2\n" + "0 0 0\n" * 7 + "0 0 0x1\n",
    "row_comma": "LUT_3D_SIZE 2\n" + "0 0 0\n" * 7 + "0 0 0,5\n",
    "row_lone_point": "LUT_3D_SIZE 2\n" + "0 0 0\n" * 7 + "0 0 .\n",
    "row_lone_exponent": "LUT_3D_SIZE 2\n" + "0 0 0\n" * 7 + "0 0 1e\n",
    "row_nan": "LUT_3D_SIZE 2\n" + "0 0 0\n" * 7 + "0 0 nan\n",
    "value_1e6": "LUT_3D_SIZE 2\n" + "0 0 0\n" * 7 + "0 0 1000000\n",
    "value_minus_1e6": "LUT_3D_SIZE 2\n" + "0 0 0\n" * 7 + "0 0 -1e6\n",
    "value_1e20": "LUT_3D_SIZE 2\n" + "0 0 0\n" * 7 + "0 0 1e20\n",
    "domain_equal": "LUT_3D_SIZE 2\nDOMAIN_MIN 0 0 0\nDOMAIN_MAX 1 0 1\n" + "0 0 0\n" * 8,
    "domain_reversed": "LUT_3D_SIZE 2\nDOMAIN_MIN 0 0 2\nDOMAIN_MAX 1 1 1\n" + "0 0 0\n" * 8,
    "domain_of_two": "LUT_3D_SIZE 2\nDOMAIN_MIN 0 0\n" + "0 0 0\n" * 8,
    "input_range_not_unit": "LUT_3D_SIZE 2\nLUT_3D_INPUT_RANGE 0 2\n" + "0 0 0\n" * 8,
    "input_range_reversed": "LUT_3D_SIZE 2\nLUT_3D_INPUT_RANGE 1 0\n" + "0 0 0\n" * 8,
    "keyword_unknown": "LUT_3D_SIZE 2\nLUT_IN_VIDEO_RANGE\n" + "0 0 0\n" * 8,
    "keyword_behind_rows": "LUT_3D_SIZE 2\n" + "0 0 0\n" * 8 + "DOMAIN_MAX 1 1 1\n",
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_parser_refuses(E, name):
    with pytest.raises(ValueError):
        R.parse_cube(REFUSED[name])
    with pytest.raises(E.EncoderError):
        E.parse_cube(REFUSED[name])


def test_parser_refuses_null_and_too_little_room(E):
    L = E.load()
    text = ("LUT_3D_SIZE 2\n" + "0 0 0\n" * 8).encode()
    nodes, N = np.zeros(8, np.uint32), C.c_int(0)
    assert L.mi355enc_lut3d_parse_cube(text, len(text), nodes.ctypes.data, 8, C.byref(N)) == 0 and N.value == 2
    assert L.mi355enc_lut3d_parse_cube(text, len(text), nodes.ctypes.data, 7, C.byref(N)) == E.ERR_ARG
    assert L.mi355enc_lut3d_parse_cube(None, 0, nodes.ctypes.data, 8, C.byref(N)) == E.ERR_ARG
    assert L.mi355enc_lut3d_parse_cube(text, len(text), None, 8, C.byref(N)) == E.ERR_ARG
    assert L.mi355enc_lut3d_parse_cube(text, len(text), nodes.ctypes.data, 8, None) == E.ERR_ARG
    with pytest.raises(ValueError):
        R.parse_cube(text, cap=7)


COMMA_LOCALES = ("de_DE.UTF-8", "de_DE.utf8", "fr_FR.UTF-8", "fr_FR.utf8", "de_DE", "fr_FR", "nl_NL.UTF-8", "es_ES.UTF-8", "it_IT.UTF-8", "pt_BR.UTF-8", "ru_RU.UTF-8")


def comma_locale():
    saved = locale.setlocale(locale.LC_NUMERIC)
    try:
        for name in COMMA_LOCALES:
            try:
                locale.setlocale(locale.LC_NUMERIC, name)
            except locale.Error:
                continue
            if locale.localeconv()["decimal_point"] == ",":
                return name
        return None
    finally:
        locale.setlocale(locale.LC_NUMERIC, saved)


def test_parser_ignores_a_comma_locale(E):
    name = comma_locale()
    if name is None:
        pytest.skip("no locale with a decimal comma is installed on this machine (tried %s)" % ", ".join(COMMA_LOCALES))
    code = ("import locale, sys, ctypes\n"
            "locale.setlocale(locale.LC_ALL, %r)\n"
            "ctypes.CDLL(None).setlocale(1, %r.encode())\n"  # LC_NUMERIC of the C library itself
            "assert locale.localeconv()['decimal_point'] == ','\n"
            "sys.path.insert(0, %r)\n"
            "import ceracoder_amd.enc as E\n"
            "nodes, N = E.parse_cube(open(%r, 'rb').read())\n"
            "print(N, ' '.join('%%d' %% v for v in nodes))\n" % (name, name, ROOT, GOLDEN))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    want, N = R.parse_cube(open(GOLDEN, "rb").read())
    assert r.stdout.split() == [str(N)] + [str(int(v)) for v in want]
