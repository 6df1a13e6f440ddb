"""JPEG stills, the host half: the rule of tests/snapref.py pinned to libjpeg (Pillow where it is installed, and Pillow-made fixtures
everywhere), the product's writer against tests/jpegref.py's decoder, the product's own decoder and Pillow, the proven size bound, the arithmetic limits, and
the reciprocals the device divides with.  No device."""
import importlib.util
import io
import os

import numpy as np
import pytest

from tests import jpegref, snapref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "snapshot")
HAVE_PIL = importlib.util.find_spec("PIL") is not None
QUALITIES = (10, 50, 75, 90, 100)


def _check_grey(data, plane, table):
    """a grey JPEG made by libjpeg from `plane` holds the rule's table and the rule's levels"""
    hdr, coefs, qt = jpegref.entropy_decode(data)
    h, w = plane.shape
    assert (hdr["width"], hdr["height"], hdr["components"]) == (w, h, 1)
    assert np.array_equal(qt[0], table)
    want = snapref.quantise(snapref.plane_coefs(plane), table)
    assert np.array_equal(coefs[0], want), int(np.abs(coefs[0] - want).max())


# ------------------------------------------------------------------------------------------------ 1: the pin to libjpeg
@pytest.mark.skipif(not HAVE_PIL, reason="Pillow is not installed")
@pytest.mark.parametrize("w,h", [(72, 40), (64, 48), (41, 23), (256, 144)])
def test_rule_equals_libjpeg_through_pillow(w, h):
    from PIL import Image
    for kind in ("textured", "noise", "saturated"):
        y, _ = snapref.picture((w + 1) & ~1, (h + 1) & ~1, kind, seed=4)
        p = np.ascontiguousarray(y[:h, :w])
        for q in QUALITIES:
            t = snapref.tables(q)
            buf = io.BytesIO()
            Image.fromarray(p, "L").save(buf, "JPEG", quality=q)
            _check_grey(buf.getvalue(), p, t[0])
            buf = io.BytesIO()
            Image.fromarray(p, "L").save(buf, "JPEG", qtables=[[int(v) for v in t[1]]])  # the chroma table (qtables= takes natural order)
            _check_grey(buf.getvalue(), p, t[1])


def test_rule_equals_libjpeg_on_the_committed_fixtures():
    """the same comparison where Pillow is absent: grey JPEGs Pillow made (tests/golden/snapshot/make_golden.py), and their planes"""
    names = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".jpg"))
    assert len(names) >= 5
    for name in names:
        q = int(name.split("_q")[1].split("_")[0])
        plane = np.load(os.path.join(GOLDEN, name + ".plane.npy"))
        assert plane.shape[0] <= 40 and plane.shape[1] <= 72
        _check_grey(open(os.path.join(GOLDEN, name + ".jpg"), "rb").read(), plane, snapref.tables(q)[1 if name.endswith("chroma") else 0])


def test_product_tables_equal_the_rule(E):
    for q in range(1, 101):
        assert np.array_equal(E.snapshot_tables(q), snapref.tables(q)), q
    for q in (0, 101, -3):
        with pytest.raises(E.EncoderError):
            E.snapshot_tables(q)


# ------------------------------------------------------------------------------------------------ 2: the writer
@pytest.mark.parametrize("w,h", [(16, 16), (72, 40), (50, 34), (9, 5)])
def test_writer_round_trips(E, w, h):
    """the file decodes -- by tests/jpegref.py, by the product's own decoder (even sizes), by Pillow -- to the levels, tables and size it was written from, and is
    byte for byte tests/snapref.write's"""
    for q in (1, 50, 100):
        for kind in ("textured", "noise"):
            s = 8 if (w, h) == (9, 5) else 1  # 9 x 5: 72 x 40 reduced by 8 -- odd luma, 5 x 3 chroma
            y, uv = snapref.picture(w * s if s > 1 else w, h * s if s > 1 else h, kind, seed=q)
            lv, qt, (ow, oh) = snapref.levels(y, uv, s, q)
            assert (ow, oh) == (w, h)
            data = E.snapshot_write(lv, qt, ow, oh)
            assert data == snapref.write(lv, qt, ow, oh)
            assert len(data) <= E.snapshot_max_bytes(ow, oh)
            hdr, got, gqt = jpegref.entropy_decode(data)
            assert (hdr["width"], hdr["height"], hdr["components"], hdr["hs"], hdr["vs"], hdr["restart_interval"]) == (ow, oh, 3, 2, 2, 0)
            assert np.array_equal(gqt[0], qt[0]) and np.array_equal(gqt[1], qt[1]) and np.array_equal(gqt[2], qt[1])
            assert all(np.array_equal(a, b) for a, b in zip(got, lv))
            if not (ow | oh) & 1:
                info, mine, mqt = E.jpeg_entropy_decode(data)
                assert (info.width, info.height, info.components, info.hs, info.vs) == (ow, oh, 3, 2, 2)
                assert all(np.array_equal(a, b) for a, b in zip(mine, lv)) and np.array_equal(mqt.reshape(3, 64)[:2], qt)
            if HAVE_PIL:
                from PIL import Image
                im = Image.open(io.BytesIO(data))
                assert im.size == (ow, oh) and im.format == "JPEG"
                im.draft("YCbCr", im.size)
                ycc = np.asarray(im)
                # Pillow's decoder (libjpeg-turbo, ISLOW inverse transform) upsamples 4:2:0 chroma with its "fancy" triangle filter, which is no part of
                # this rule: the luma plane is compared, chroma is not.
                want = jpegref.planes_from_coefs(lv, np.vstack([qt, qt[1:]]), ow + (ow & 1), oh + (oh & 1), 2, 2)[0][:oh, :ow]
                assert im.mode == "YCbCr" and np.array_equal(ycc[..., 0], want)


def _extreme_levels(ow, oh, sign):
    """nothing but the largest levels Huffman coding expresses: every AC +-1023 (alternating, so that no run is ever coded), DC alternating +-1020 (differences of 11 bits)"""
    out = []
    for bw, bh in snapref.layout(ow, oh):
        lv = np.empty((bh, bw, 64), np.int16)
        lv[..., 1:] = (1023 * sign * np.where(np.arange(63) & 1, -1, 1)).astype(np.int16)
        n = np.arange(bh * bw).reshape(bh, bw)
        lv[..., 0] = np.where(n & 1, -1020, 1020) * sign
        out.append(lv.reshape(bh, bw, 8, 8))
    return out


@pytest.mark.parametrize("ow,oh", [(16, 16), (50, 34)])
def test_max_bytes_holds_on_nothing_but_extreme_levels(E, ow, oh):
    qt = snapref.tables(100)
    for sign in (1, -1):
        lv = _extreme_levels(ow, oh, sign)
        data = E.snapshot_write(lv, qt, ow, oh)
        assert len(data) <= E.snapshot_max_bytes(ow, oh)
        assert len(data) > E.snapshot_max_bytes(ow, oh) // 3  # (the bound is not idle: byte stuffing may double a block)
        assert all(np.array_equal(a, b) for a, b in zip(jpegref.entropy_decode(data)[1], lv))
    lv = [np.full_like(c, -1) for c in lv]  # all bits set: the most 0xFF bytes
    assert len(E.snapshot_write(lv, qt, ow, oh)) <= E.snapshot_max_bytes(ow, oh)


def test_writer_refuses_what_huffman_cannot_code_and_reports_the_size_it_needs(E):
    y, uv = snapref.picture(50, 34, "textured")
    lv, qt, (ow, oh) = snapref.levels(y, uv, 1, 75)
    data = E.snapshot_write(lv, qt, ow, oh)
    for cap in (0, 1, 100, 622, 623, len(data) - 1):
        assert E.snapshot_write(lv, qt, ow, oh, cap=cap, want_len=True) == (-5, len(data)), cap
    assert E.snapshot_write(lv, qt, ow, oh, cap=len(data), want_len=True) == (0, len(data))
    bad = [c.copy() for c in lv]
    bad[1][0, 0, 3, 3] = 1024
    assert E.snapshot_write(bad, qt, ow, oh, want_len=True)[0] == -1
    bad = [c.copy() for c in lv]
    bad[0][0, 0, 0, 0], bad[0][0, 1, 0, 0] = -1024, 1024
    assert E.snapshot_write(bad, qt, ow, oh, want_len=True)[0] == -1
    assert E.snapshot_write(lv, np.zeros((2, 64), np.uint16), ow, oh, want_len=True)[0] == -1
    assert E.snapshot_max_bytes(0, 5) == 0 and E.snapshot_max_bytes(70000, 5) == 0


# ------------------------------------------------------------------------------------------------ 3: the extremes
@pytest.mark.parametrize("kind", ["saturated", "noise"])
def test_extremes_at_quality_100_stay_inside_what_baseline_huffman_codes(E, kind):
    """a 0 / 255 checkerboard (and random 0 / 255) and per-sample noise at quality 100: |AC| <= 1023, DC differences within 11 bits, no intermediate of the transform
    leaves 32 bits, every numerator of the quantiser stays below 8192 + 1020 + 1 -- and the file round-trips"""
    y, uv = snapref.picture(64, 48, kind, seed=8)
    if kind == "saturated":
        y[:8, :8], y[8:16, :8], y[:8, 8:16] = 0, 255, 255  # flat blocks at both ends: the DC limits and the largest DC difference
    planes = snapref.reduced_planes(y, uv, 1)
    lv, qt, peak = snapref.levels_of_planes(planes, 100)
    assert peak < 2 ** 31
    for c, p in zip(lv, planes):
        bh, bw = c.shape[:2]
        co = snapref.fdct(snapref.plane_blocks(p, bw, bh))[0]
        assert np.abs(co).max() <= 8192
        flat = c.reshape(-1, 64).astype(int)
        assert np.abs(flat[:, 1:]).max() <= 1023 and np.abs(flat[:, 0]).max() <= 1024
    if kind == "saturated":
        assert lv[0][0, 0, 0, 0] == -1024 and lv[0][1, 0, 0, 0] == 1016 and np.abs(lv[0].reshape(-1, 64)[:, 1:]).max() > 500
    data = E.snapshot_write(lv, qt, 64, 48)
    assert all(np.array_equal(a, b) for a, b in zip(jpegref.entropy_decode(data)[1], lv))


# ------------------------------------------------------------------------------------------------ 4: the reciprocals
def test_reciprocal_equals_division_exhaustively(E):
    """the kernel computes (|c| + 4 q) / (8 q) as ((|c| + 4 q) * m) >> 32 with the host's m: every divisor, every numerator from 0 to 8192 + 1020"""
    n = np.arange(0, 8192 + 1020 + 1, dtype=np.uint64)
    for q in range(1, 256):
        m = E.snapshot_reciprocal(q)
        assert 0 < m < 2 ** 32 and m == -(-2 ** 32 // (8 * q))
        assert np.array_equal((n * np.uint64(m)) >> np.uint64(32), n // np.uint64(8 * q)), q
    assert E.snapshot_reciprocal(0) == 0 and E.snapshot_reciprocal(256) == 0
