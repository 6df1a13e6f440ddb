"""MJPEG input, host half (no device): mi355enc_jpeg_info / mi355enc_jpeg_entropy_decode against the coefficients the
writer of tests/jpegref.py coded, the refused stream kinds, robustness against truncated and corrupted pictures (in process, and under
ASan + UBSan through san_jpeg_driver.c), and tests/jpegref.py itself against an independent decoder (Pillow) where one is installed."""
import ctypes as C
import glob
import io
import json
import os
import subprocess

import numpy as np
import pytest

from ceracoder_amd import enc as E
from tests import jpegref as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ceracoder_amd", "csrc")
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "jpeg", "*.jpg")))
ERR_ARG, ERR_OVERFLOW = -1, -5  # include/mi355enc.h
SHAPES = [(16, 16, 0), (40, 24, 0), (72, 40, 2)]  # width, height, restart interval in MCUs
FINE = (J.scaled_q(J.Q_LUMA, 10), J.scaled_q(J.Q_CHROMA, 10))  # small quantisers: large coefficients, long codes, stuffed bytes


def _same(got, want):
    return len(got) == len(want) and all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(got, want))


def _rc(data, cap=None):
    """return code of the decode alone, coefficient room `cap` int16 (default: what the header asks for, at most 2^22)"""
    L = E.load()
    buf = np.frombuffer(bytes(data), np.uint8)
    info = E.JpegInfo()
    r = L.mi355enc_jpeg_info(buf.ctypes.data if buf.size else None, buf.size, C.byref(info))
    if r:
        return r, None
    need = sum(bw * bh for bw, bh in E.jpeg_layout(info)) * 64
    cap = min(need, 1 << 22) if cap is None else cap
    guard = 256
    coef = np.full(cap + 2 * guard, 0x5A5A, np.int16)
    qt = np.zeros((3, 64), np.uint16)
    r = L.mi355enc_jpeg_entropy_decode(buf.ctypes.data, buf.size, coef[guard:].ctypes.data, cap, qt.ctypes.data, None)
    assert (coef[:guard] == 0x5A5A).all() and (coef[guard + cap:] == 0x5A5A).all(), "wrote outside the coefficient buffer"
    return r, info


@pytest.mark.parametrize("w,h,dri", SHAPES)
@pytest.mark.parametrize("sampling", ["grey", "420", "422", "444"])
def test_entropy_decode_returns_the_writers_coefficients(sampling, w, h, dri):
    planes = J.subsample(*J.picture(w, h, w + h), sampling)
    nc, hs, vs = J.SAMPLING[sampling]
    for dht in (True, False):
        for split in (False, True):
            data, coefs = J.write_jpeg(planes, sampling, dri=dri, dht=dht, split_tables=split, fill=split)
            info, got, qt = E.jpeg_entropy_decode(data)
            assert _same(got, coefs)
            assert (info.width, info.height, info.components, info.hs, info.vs, info.restart_interval, info.has_dht) == (w, h, nc, hs, vs, dri, int(dht))
            assert np.array_equal(qt[0].ravel(), J.Q_LUMA) and (nc == 1 or np.array_equal(qt[1].ravel(), J.Q_CHROMA) and np.array_equal(qt[2], qt[1]))
            hdr, ref, rq = J.entropy_decode(data)  # the restatement reads the same picture the same way
            assert _same(ref, coefs) and np.array_equal(rq, qt.reshape(3, 64))


@pytest.mark.parametrize("sampling", ["grey", "420", "422", "444"])
def test_entropy_decode_with_generated_16_bit_tables_and_stuffed_bytes(sampling):
    tables = J.generated_tables(0xC0DE)
    assert max(l for t in tables.values() for l, n in enumerate(t[0], 1) if n) == 16
    planes = J.subsample(*J.picture(72, 40, 9, noise=120), sampling)
    for dri in (0, 2):
        data, coefs = J.write_jpeg(planes, sampling, qts=FINE, tables=tables, dri=dri)
        info, got, qt = E.jpeg_entropy_decode(data)
        assert _same(got, coefs) and np.array_equal(qt[0].ravel(), FINE[0])
        assert max(int(np.abs(c).max()) for c in coefs) > 255


def test_long_zero_runs_and_extreme_values_survive():
    """ZRL symbols, a coefficient at position 63, the extreme AC and DC values, and stuffed 0xFF bytes forced by content: the typical luminance AC code of
    run 15 / size 10 is fifteen 1 bits and a 0, and the value 1023 behind it ten more 1 bits"""
    co = [np.zeros((2, 2, 8, 8), np.int16), np.zeros((1, 1, 8, 8), np.int16), np.zeros((1, 1, 8, 8), np.int16)]
    co[0][0, 0, 7, 7] = -1023
    co[0][0, 1, 0, 0], co[0][0, 1, 4, 4] = 1023, 1023
    co[0][1, 0, 0, 0] = -1024
    co[1][0, 0, 7, 6], co[2][0, 0, 0, 1] = 1, -1
    co[0][1, 1].reshape(64)[J.NATURAL[16]] = 1023
    co[0][1, 1].reshape(64)[J.NATURAL[32]] = 1023
    for dht in (True, False):
        data = J.encode_coefs(co, 16, 16, "420", dht=dht)
        assert data[J.parse(data)["scan"]:].count(b"\xff\x00") >= 2
        _, got, _ = E.jpeg_entropy_decode(data)
        assert _same(got, co)


def test_too_little_room_is_an_overflow():
    data, coefs = J.write_jpeg(J.subsample(*J.picture(40, 24, 1), "420"), "420")
    need = sum(c.size for c in coefs)
    assert _rc(data, need - 1)[0] == ERR_OVERFLOW
    assert _rc(data, need)[0] == 0


REFUSED = {
    "progressive": dict(sof_marker=0xC2), "lossless": dict(sof_marker=0xC3), "arithmetic": dict(sof_marker=0xC9), "progressive arithmetic": dict(sof_marker=0xCA),
    "12-bit": dict(precision=12), "four components": dict(extra_component=True), "non-interleaved": dict(scan_components=1),
    "sampling 1x2": dict(luma_hv=0x12), "sampling 4x1": dict(luma_hv=0x41), "16-bit quantisation tables": dict(pq=1),
}


@pytest.mark.parametrize("kind", sorted(REFUSED))
def test_refused_stream_kinds(kind):
    planes = J.subsample(*J.picture(16, 16, 2), "420")
    coefs = J.quantise(planes, "420", (J.Q_LUMA, J.Q_CHROMA))
    good = J.encode_coefs(coefs, 16, 16, "420")
    assert _rc(good)[0] == 0
    bad = J.encode_coefs(coefs, 16, 16, "420", **REFUSED[kind])
    assert _rc(bad)[0] == ERR_ARG
    with pytest.raises(J.Refused):
        J.parse(bad)
    L = E.load()
    assert L.mi355enc_jpeg_info(None, 0, C.byref(E.JpegInfo())) == ERR_ARG


def _corrupt_block_cases():
    """pictures whose entropy-coded data breaks one rule each"""
    t = dict(J.STD_TABLES)
    cases = {}
    # a DC size of 12 and an AC size of 11: tables that hold such symbols, and data that uses them
    t12 = dict(t)
    t12[(0, 0)] = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0], list(range(13)))
    co = [np.zeros((1, 1, 8, 8), np.int16)]
    big = J.encode_coefs(co, 8, 8, "grey", tables=t12)
    cases["DC size 12"] = _with_symbols(co, t12, dc_size=12)
    t11 = dict(t)
    t11[(1, 0)] = (J.STD_AC_L[0][:15] + [J.STD_AC_L[0][15] + 1], J.STD_AC_L[1] + [0x0B])
    cases["AC size 11"] = _with_symbols(co, t11, ac_symbol=0x0B)
    cases["run past 63"] = _with_symbols(co, t, ac_symbol=0xF1, repeat=5)
    assert _rc(big)[0] == 0
    return cases


def _with_symbols(co, tables, dc_size=0, ac_symbol=None, repeat=1):
    """an 8 x 8 grey picture whose one block is written symbol by symbol"""
    good = J.encode_coefs(co, 8, 8, "grey", tables=tables)
    head = good[:J.parse(good)["scan"]]
    codes = {k: J.huff_codes(*v) for k, v in tables.items()}
    b = J._Bits()
    b.put(*codes[(0, 0)][dc_size])
    if dc_size:
        b.put((1 << dc_size) - 1, dc_size)
    if ac_symbol is not None:
        for _ in range(repeat):
            b.put(*codes[(1, 0)][ac_symbol])
            b.put(1, ac_symbol & 15)
    b.put(*codes[(1, 0)][0])
    b.flush()
    return head + bytes(b.out) + b"\xff\xd9"


def test_corrupt_entropy_coded_data_is_refused():
    for name, data in _corrupt_block_cases().items():
        assert _rc(data)[0] == ERR_ARG, name
        with pytest.raises(J.Refused):
            J.entropy_decode(data)
    planes = J.subsample(*J.picture(72, 40, 4), "422")
    data, _ = J.write_jpeg(planes, "422", dri=2)
    scan = J.parse(data)["scan"]
    first = data.index(b"\xff\xd0", scan)
    assert _rc(data[:first] + b"\xff\xd1" + data[first + 2:])[0] == ERR_ARG      # RSTn out of order
    assert _rc(data[:first] + data[first + 2:])[0] == ERR_ARG                    # RSTn missing
    assert _rc(data[:len(data) - 12])[0] == ERR_ARG                              # data ends before the last MCU
    undefined = dict(J.STD_TABLES)
    undefined[(1, 0)] = ([0, 2] + [0] * 14, [0x00, 0x01])                        # two AC codes, `00` and `01`: every prefix that starts with 1 is undefined
    co = [np.zeros((1, 1, 8, 8), np.int16)]
    good = J.encode_coefs(co, 8, 8, "grey", tables=undefined)
    assert _rc(good)[0] == 0
    b = J._Bits()
    b.put(*J.huff_codes(*J.STD_DC_L)[0])
    b.put(0xFFFE, 16)
    b.flush()
    assert _rc(good[:J.parse(good)["scan"]] + bytes(b.out) + b"\xff\xd9")[0] == ERR_ARG
    # a DC predictor that leaves int16: differences of +2047 block after block
    co = [np.zeros((1, 20, 8, 8), np.int16)]
    data = J.encode_coefs(co, 160, 8, "grey")
    head = data[:J.parse(data)["scan"]]
    codes = {k: J.huff_codes(*v) for k, v in J.STD_TABLES.items()}
    b = J._Bits()
    for _ in range(20):
        b.put(*codes[(0, 0)][11])
        b.put(2047, 11)
        b.put(*codes[(1, 0)][0])
    b.flush()
    assert _rc(head + bytes(b.out) + b"\xff\xd9")[0] == ERR_ARG


@pytest.fixture(scope="module")
def victim(tmp_path_factory):
    data, _ = J.write_jpeg(J.subsample(*J.picture(40, 24, 6), "420"), "420", dri=2)
    p = tmp_path_factory.mktemp("jpeg") / "victim.jpg"
    p.write_bytes(data)
    return data, str(p)


def test_truncation_at_every_length(victim):
    data, _ = victim
    assert _rc(data)[0] == 0
    codes = [_rc(data[:n])[0] for n in range(len(data) + 1)]
    assert all(c in (0, ERR_ARG) for c in codes)
    assert all(c == ERR_ARG for c in codes[:len(data) - 8])  # what is cut before the last MCU's data cannot decode


def _lcg_cases(size, seed, n):
    x, out = seed, []
    for _ in range(n):
        x = (x * 6364136223846793005 + 1442695040888963407) & (2 ** 64 - 1)
        pos = (x >> 33) % size
        x = (x * 6364136223846793005 + 1442695040888963407) & (2 ** 64 - 1)
        out.append((pos, x >> 56))
    return out


def test_seeded_single_byte_corruptions(victim):
    data, _ = victim
    ok = err = 0
    for pos, val in _lcg_cases(len(data), 0x1234, 2000):
        bad = bytearray(data)
        bad[pos] = val
        r, _ = _rc(bytes(bad))
        assert r in (0, ERR_ARG, ERR_OVERFLOW)  # (a corrupt header may announce a picture larger than the room offered)
        ok, err = ok + (r == 0), err + (r != 0)
    assert ok and err


@pytest.fixture(scope="module")
def san_jpeg():
    r = subprocess.run(["make", "-C", CSRC, "san/san_jpeg"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return os.path.join(CSRC, "san", "san_jpeg")


def test_the_same_cases_are_clean_under_asan_and_ubsan(san_jpeg, victim):
    data, path = victim
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    want = {"trunc": None, "fuzz": None}
    codes = [_rc(data[:n])[0] for n in range(len(data) + 1)]
    want["trunc"] = (sum(c == 0 for c in codes), sum(c != 0 for c in codes))
    res = []
    for pos, val in _lcg_cases(len(data), 0x1234, 2000):
        bad = bytearray(data)
        bad[pos] = val
        res.append(_rc(bytes(bad))[0])
    want["fuzz"] = (sum(c == 0 for c in res), sum(c != 0 for c in res))
    for mode, args in (("decode", []), ("trunc", []), ("fuzz", ["0x1234", "2000"])):
        r = subprocess.run([san_jpeg, mode, path] + args, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
        out = json.loads(r.stdout)
        if mode == "decode":
            assert out["rc"] == 0
        else:
            assert (out["ok"], out["err"]) == want[mode]  # the sanitized decoder and the shipped one take every case the same way


# ------------------------------------------------------------------------------------------------ the restatement against an independent decoder
def _pil_luma(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.draft("YCbCr", im.size)
    im.load()
    return np.asarray(im) if im.mode == "L" else np.asarray(im)[..., 0]


@pytest.mark.parametrize("sampling", ["grey", "420", "422", "444"])
def test_reference_luma_equals_pillow_on_the_writers_pictures(sampling):
    pytest.importorskip("PIL")
    for w, h, dri in SHAPES:
        for qts in ((J.Q_LUMA, J.Q_CHROMA), FINE):
            data, _ = J.write_jpeg(J.subsample(*J.picture(w, h, 11), sampling), sampling, qts=qts, dri=dri)
            assert np.array_equal(_pil_luma(data), J.decode(data)[1][0])


@pytest.mark.parametrize("quality,optimize,subsampling", [(50, False, 2), (90, True, 2), (90, False, 1), (50, True, 0), (90, True, 1)])
def test_reference_luma_equals_pillow_on_pillow_written_pictures(quality, optimize, subsampling):
    pytest.importorskip("PIL")
    from PIL import Image
    y, u, v = J.picture(72, 40, quality)
    b = io.BytesIO()
    Image.fromarray(np.stack([y, u, v], axis=-1), "YCbCr").save(b, "JPEG", quality=quality, optimize=optimize, subsampling=subsampling)
    data = b.getvalue()
    fmt, planes = J.decode(data)
    assert fmt == {2: J.FMT_I420, 1: J.FMT_Y42B, 0: J.FMT_Y444}[subsampling]
    assert np.array_equal(_pil_luma(data), planes[0])
    _, got, qt = E.jpeg_entropy_decode(data)
    _, ref, rq = J.entropy_decode(data)
    assert _same(got, ref) and np.array_equal(qt.reshape(3, 64), rq)


def test_golden_files_decode_like_the_reference():
    """Pillow-written pictures kept under tests/golden/jpeg (made by make_golden.py there): real-encoder files for machines without Pillow"""
    assert len(GOLDEN) >= 4
    for path in GOLDEN:
        data = open(path, "rb").read()
        assert len(data) <= 8192
        _, got, qt = E.jpeg_entropy_decode(data)
        _, ref, rq = J.entropy_decode(data)
        assert _same(got, ref) and np.array_equal(qt.reshape(3, 64), rq), path
        want = np.load(path[:-4] + ".luma.npy")  # the luma Pillow decoded when the file was made
        assert np.array_equal(J.decode(data)[1][0], want), path
