"""CPU: the containers of tests/inputref.py, the evidence that the GPU input-path tests are sensitive, and the strided-array rule of
ceracoder_amd/enc.py.

Sensitivity: tests/test_input_paths_gpu.py expects the stream the oracle makes of the clean visible pictures -- the stream of the properly
replicated coded picture.  Here the oracle alone, at the coded size, is fed that picture and the picture a reader without a clamp would have
taken from the container (poison, or in the "bench" layout the chroma plane, in the rows below the visible height; poison in the columns
behind the visible width): the access units of the IDR picture and of the first P picture differ for every padded geometry the GPU tests use.
A kernel that read what it must not would therefore not produce the expected stream."""
import ctypes as C

import numpy as np
import pytest

from ceracoder_amd import synth
from tests import inputref as R
from tests.util import pad_planes


def _pic(w, h, seed=1):
    g = np.random.default_rng(seed)
    return g.integers(0, 256, (h, w), dtype=np.uint8), g.integers(0, 256, (h // 2, w), dtype=np.uint8)


# ---- the helpers
@pytest.mark.parametrize("layout", R.LAYOUTS)
@pytest.mark.parametrize("w,h,pad", [(320, 180, 0), (320, 180, 64), (322, 182, 2), (16, 16, 16), (18, 18, 3)])
def test_visible_view_of_every_layout_is_the_picture(layout, w, h, pad):
    y, uv = _pic(w, h)
    stride = 2 * w if layout == "interleaved_rows" else w + pad
    buf, yo, uo = R.container(y, uv, stride, layout=layout, seed=7)
    assert np.array_equal(R.visible(buf, yo, h, w, stride), y) and np.array_equal(R.visible(buf, uo, h // 2, w, stride), uv)
    assert yo >= R.MIN_GUARD and uo >= R.MIN_GUARD and buf.size - max(yo + h * stride, uo + h // 2 * stride) >= R.MIN_GUARD
    assert yo % 16 == 0 and (uo % 16 == 0 or (layout == "bench" and stride % 16))
    if layout == "bench":
        assert uo == yo + h * stride
    if layout == "uv_first":
        assert uo < yo
    # everything that is not a visible sample is the seed's noise
    mask = np.ones(buf.size, bool)
    for off, rows in ((yo, h), (uo, h // 2)):
        mask[(off + np.arange(rows)[:, None] * stride + np.arange(w)[None, :]).ravel()] = False
    assert np.array_equal(buf[mask], R.noise(buf.size, 7)[mask])
    if layout == "interleaved_rows":
        assert np.array_equal(R.visible(buf, yo + w, h, w, stride), R.visible(R.noise(buf.size, 7), yo + w, h, w, stride))


def test_separate_strides_and_an_odd_address():
    y, uv = _pic(320, 180)
    buf, yo, uo = R.container(y, uv, 323, layout="apart", seed=3, offset=1)
    assert yo % 16 == 1 and uo % 16 == 1 and np.array_equal(R.visible(buf, yo, 180, 320, 323), y) and np.array_equal(R.visible(buf, uo, 90, 320, 323), uv)
    buf, yo, uo = R.container(y, uv, 336, layout="apart", seed=3, uv_stride=384)
    assert np.array_equal(R.visible(buf, yo, 180, 320, 336), y) and np.array_equal(R.visible(buf, uo, 90, 320, 384), uv)


def test_poison_is_fresh_for_every_seed():
    y, uv = _pic(64, 48)
    a, b = R.container(y, uv, 80, seed=1)[0], R.container(y, uv, 80, seed=2)[0]
    assert a.size == b.size and (a != b).sum() > 0.99 * (a.size - 64 * 72)  # (all but the 64 x 72 visible samples)


def test_poison_assertions_fire_on_replicated_padding():
    w, h, stride = 322, 182, 336
    y, uv = _pic(w, h)
    buf, yo, uo = R.container(y, uv, stride, layout="apart", seed=5)
    R.assert_poisoned(buf, yo, uo, y, uv, stride)
    rows = buf.copy()  # the row below the luma plane replicated
    rows[yo + h * stride:yo + h * stride + w] = y[h - 1]
    with pytest.raises(AssertionError, match="below a plane"):
        R.assert_poisoned(rows, yo, uo, y, uv, stride)
    crow = buf.copy()  # ... below the chroma plane
    crow[uo + (h // 2 + 3) * stride:uo + (h // 2 + 3) * stride + w] = uv[h // 2 - 1]
    with pytest.raises(AssertionError, match="below a plane"):
        R.assert_poisoned(crow, yo, uo, y, uv, stride)
    cols = buf.copy()  # one luma row's tail replicated
    cols[yo + 17 * stride + w:yo + 18 * stride] = y[17, w - 1]
    with pytest.raises(AssertionError, match="row 17"):
        R.assert_poisoned(cols, yo, uo, y, uv, stride)
    ccol = buf.copy()  # one chroma row's tail: the last Cb, Cr pair repeated
    ccol[uo + 5 * stride + w:uo + 6 * stride] = np.tile(uv[5, w - 2:w], (stride - w) // 2)
    with pytest.raises(AssertionError, match="row 5"):
        R.assert_poisoned(ccol, yo, uo, y, uv, stride)


# ---- sensitivity, on the oracle alone
# (geometry, stride, layout) of every GPU case group whose coded picture has padding: in place (1920 x 1080 as the bench lays it out, 320 x 180), copied
# (322 x 182, 50 x 34, 320 x 180 at an odd stride), host rows (322 x 182, 1920 x 1080, 18 x 18)
PADDED = [(1920, 1080, 1920, "bench"), (1920, 1080, 1984, "bench"), (1920, 1080, 1984, "apart"), (1920, 1080, 3840, "interleaved_rows"),
          (320, 180, 320, "bench"), (320, 180, 384, "bench"), (320, 180, 336, "uv_first"), (320, 180, 323, "apart"),
          (322, 182, 324, "apart"), (322, 182, 386, "bench"), (50, 34, 53, "apart"), (50, 34, 64, "bench"), (18, 18, 20, "apart"), (18, 18, 82, "bench")]


@pytest.mark.parametrize("w,h,stride,layout", PADDED, ids=lambda v: str(v))
def test_poison_in_place_of_replication_changes_the_oracle_stream(oracle, w, h, stride, layout):
    W, H = (w + 15) // 16 * 16, (h + 15) // 16 * 16
    names = ["all", "p_only"] + (["rows", "cols"] if H > h and W > w else [])  # p_only: a clean IDR picture, then the P picture read without clamps
    clean = oracle.Encoder(W, H, gop=4, threads=8, scenecut=False)
    encs = {k: oracle.Encoder(W, H, gop=4, threads=8, scenecut=False) for k in names}
    for i, (y, uv) in enumerate(synth.s2_frames(w, h, 2)):
        buf, yo, uo = R.container(y, uv, stride, layout=layout, seed=100 + i)
        py, puv = pad_planes(y, uv)
        ry, ruv = R.coded_read(buf, yo, H, W, stride), R.coded_read(buf, uo, H // 2, W, stride)
        assert np.array_equal(ry[:h, :w], y) and np.array_equal(ruv[:h // 2, :w], uv)
        rows_y, rows_uv, cols_y, cols_uv = py.copy(), puv.copy(), py.copy(), puv.copy()
        rows_y[h:], rows_uv[h // 2:] = ry[h:], ruv[h // 2:]
        cols_y[:h, w:], cols_uv[:h // 2, w:] = ry[:h, w:], ruv[:h // 2, w:]
        pics = {"all": (ry, ruv), "p_only": (ry, ruv) if i else (py, puv), "rows": (rows_y, rows_uv), "cols": (cols_y, cols_uv)}
        qp = R.QPS[i]  # (the QPs of the GPU cases' first two pictures)
        want, key = clean.encode(py, puv, qp)
        assert key == (i == 0)
        for k in names:
            au = encs[k].encode(*pics[k], qp)[0]
            assert (au != want) or (k == "p_only" and i == 0), (k, i)


def test_luma_rows_alone_and_chroma_rows_alone_change_the_stream(oracle):
    """1920 x 1080 in the bench's layout: a missed luma clamp reads the chroma plane's first eight rows, a missed chroma clamp reads four rows behind the
    chroma plane.  Each alone changes the IDR picture and the P picture."""
    w, h, W, H = 1920, 1080, 1920, 1088
    encs = [oracle.Encoder(W, H, gop=4, threads=8, scenecut=False) for _ in range(3)]
    for i, (y, uv) in enumerate(synth.s2_frames(w, h, 2)):
        buf, yo, uo = R.container(y, uv, w, layout="bench", seed=40 + i)
        py, puv = pad_planes(y, uv)
        ly = py.copy()
        ly[h:] = R.coded_read(buf, yo, H, W, w)[h:]
        assert np.array_equal(ly[h:], uv[:8])
        cuv = puv.copy()
        cuv[h // 2:] = R.coded_read(buf, uo, H // 2, W, w)[h // 2:]
        want = encs[0].encode(py, puv, 30)[0]
        assert encs[1].encode(ly, puv, 30)[0] != want and encs[2].encode(py, cuv, 30)[0] != want, i


# ---- ceracoder_amd/enc.py: a strided picture goes through as it lies
class _FakeLib:
    def __init__(self):
        self.calls = []

    def mi355enc_submit(self, h, y, ys, uv, uvs, pts, idr):
        self.calls.append(("submit", y.value, ys, uv.value, uvs, pts, idr))
        return 0

    def mi355enc_encode(self, h, y, ys, uv, uvs, pts, idr, out, cap, n, key):
        self.calls.append(("encode", y.value, ys, uv.value, uvs, pts, idr))
        return 0


def _bare_encoder(E):
    e = E.Encoder.__new__(E.Encoder)  # no library, no device: only what submit() / encode() touch
    e.L, e.h, e._out = _FakeLib(), None, np.zeros(16, np.uint8)
    return e


@pytest.mark.parametrize("call", ["submit", "encode"])
def test_strided_planes_reach_the_library_where_they_lie(E, call):
    e = _bare_encoder(E)
    w, h = 322, 182
    big_y, big_uv = np.zeros((h + 9, w + 70), np.uint8), np.zeros((h // 2 + 5, w + 2), np.uint8)
    y, uv = big_y[3:3 + h, 5:5 + w], big_uv[1:1 + h // 2, :w]
    assert not y.flags["C_CONTIGUOUS"]
    getattr(e, call)(y, uv, pts=11)
    assert e.L.calls == [(call, big_y.ctypes.data + 3 * (w + 70) + 5, w + 70, big_uv.ctypes.data + (w + 2), w + 2, 11, 0)]


@pytest.mark.parametrize("call", ["submit", "encode"])
def test_contiguous_planes_are_passed_as_before(E, call):
    e = _bare_encoder(E)
    y, uv = np.zeros((48, 64), np.uint8), np.zeros((24, 64), np.uint8)
    getattr(e, call)(y, uv, pts=2, force_idr=True)
    assert e.L.calls == [(call, y.ctypes.data, 64, uv.ctypes.data, 64, 2, 1)]


@pytest.mark.parametrize("call", ["submit", "encode"])
def test_anything_else_is_still_made_contiguous(E, call):
    """a column-strided view, another dtype, a broadcast row: copied into rows of exactly the width, as before"""
    e = _bare_encoder(E)
    wide = np.zeros((48, 128), np.uint8)
    bcast = np.broadcast_to(np.zeros((1, 64), np.uint8), (24, 64))
    for y, uv in ((wide[:, ::2], np.zeros((24, 64), np.int32)), (np.zeros((48, 64), np.float32), bcast)):
        e.L.calls.clear()
        getattr(e, call)(y, uv)
        (_, py, ys, puv, uvs, _, _), = e.L.calls
        assert (ys, uvs) == (64, 64)
        lo, hi = wide.ctypes.data, wide.ctypes.data + wide.nbytes
        assert not lo <= py < hi and puv != bcast.ctypes.data
