"""The text overlay without a device: the built-in font as the ABI hands it out against the committed ASCII art, the
style validation, and properties of the numpy restatement of the drawing rule (tests/overlayref.py) that the GPU tests compare the kernel with."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import overlayref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = "  b:  2048/ 1900 rtt:  40/ 38/ 45 bs:  12/ 10/ 14/ 11"  # the reference's statistics line, 53 characters


def _golden():
    out, cur = {}, None
    for ln in open(os.path.join(ROOT, "tests", "golden", "overlay_font.txt")).read().split():
        if ln.startswith("0x"):
            cur = int(ln, 16)
            out[cur] = []
        else:
            assert len(ln) == 8 and set(ln) <= {"#", "."}
            out[cur].append(sum(0x80 >> k for k in range(8) if ln[k] == "#"))
    return out


def test_font_is_the_committed_ascii_art(E):
    g = _golden()
    assert sorted(g) == list(range(0x20, 0x7F))
    for ch, rows in g.items():
        assert len(rows) == 16 and list(E.overlay_glyph(ch)) == rows, chr(ch)


def test_font_glyphs_are_distinct_and_leave_a_gap(E):
    cells = {ch: bytes(E.overlay_glyph(ch)) for ch in range(0x20, 0x7F)}
    assert cells[0x20] == bytes(16)
    assert all(any(c) for ch, c in cells.items() if ch != 0x20)
    assert len(set(cells.values())) == 95
    for ch, c in cells.items():
        cols = 0
        for r in c:
            cols |= r
        assert cols != 0xFF, "%r uses all eight columns" % chr(ch)
        assert not all(c), "%r uses all sixteen rows" % chr(ch)


def test_glyph_outside_the_font_is_refused(E):
    L = E.load()
    rows = (C.c_uint8 * 16)()
    for ch in (0x1F, 0x7F, 0x80, -1, 10):
        assert L.mi355enc_overlay_glyph(ch, rows) == E.ERR_ARG
    assert L.mi355enc_overlay_glyph(65, None) == E.ERR_ARG


def test_default_style_and_validation(E):
    L = E.load()
    st = E.overlay_style()
    assert (st.halign, st.valign, st.xpad, st.ypad, st.scale, st.shaded_background) == (2, 0, 16, 16, 0, 0)
    # (without a device there is no handle: that a handle accepts the valid and refuses each of these is in tests/test_overlay_gpu.py)
    for bad in (dict(halign=3), dict(halign=-1), dict(valign=3), dict(xpad=-1), dict(ypad=-2), dict(scale=9), dict(scale=-1), dict(shaded_background=2)):
        assert L.mi355enc_set_overlay_style(None, C.byref(E.overlay_style(**bad))) == E.ERR_ARG
    assert L.mi355enc_set_overlay_style(None, C.byref(st)) == E.ERR_ARG  # no handle
    assert L.mi355enc_set_overlay_text(None, b"x") == E.ERR_ARG
    with pytest.raises(TypeError):
        E.overlay_style(colour=1)


def _pic(w, h, seed=1):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w), dtype=np.uint8)


def test_auto_scale():
    assert [R.auto_scale(h) for h in (120, 720, 1080, 1440, 2160, 4320, 8192)] == [1, 1, 2, 2, 4, 8, 8]


@pytest.mark.parametrize("scale", [1, 2, 3])
def test_unshaded_drawing_is_idempotent_and_stays_inside_the_box(scale):
    y, uv = _pic(200, 112)
    st = dict(scale=scale, halign=1, valign=1)
    y1, uv1 = R.draw(y, uv, "ab\ncdef", **st)
    y2, uv2 = R.draw(y1, uv1, "ab\ncdef", **st)
    assert np.array_equal(y1, y2) and np.array_equal(uv1, uv2)
    T, O, B = R.masks("ab\ncdef", 200, 112, **st)
    assert T.any() and O.any() and not (T & O).any() and not ((T | O) & ~B).any()
    assert np.array_equal(y1[~(T | O)], y[~(T | O)])  # unshaded: only text and outline are written
    ys, uvs = R.draw(y, uv, "ab\ncdef", shaded_background=1, **st)
    assert np.array_equal(ys[~B], y[~B]) and not np.array_equal(ys, y1)
    sb = B[0::2, 0::2] | B[0::2, 1::2] | B[1::2, 0::2] | B[1::2, 1::2]
    keep = np.repeat(~sb, 2, axis=1)
    assert np.array_equal(uvs[keep], uv[keep])
    bg = B & ~T & ~O
    assert np.array_equal(ys[bg], (y[bg].astype(int) + 17) >> 1) and (ys[T] == 235).all() and (ys[O] == 16).all()


@pytest.mark.parametrize("halign,valign", [(h, v) for h in range(3) for v in range(3)])
def test_clipping_at_the_picture_edges(halign, valign):
    """a box larger than the picture in both directions, at pad 0: the origin moves to 0, the rest is cut at the visible size"""
    w, h = 64, 48
    y, uv = _pic(w, h)
    text = "\n".join(["WWWWWWWWWWWW"] * 4)  # 12 x 8 = 96 + 2 wide, 4 x 16 = 64 + 2 high
    T, O, B = R.masks(text, w, h, halign=halign, valign=valign, xpad=0, ypad=0, scale=1)
    assert B.all() and T.shape == (h, w)
    assert T[:, -1].any() or O[:, -1].any()
    yd, uvd = R.draw(y, uv, text, halign=halign, valign=valign, xpad=0, ypad=0, scale=1, shaded_background=1)
    assert yd.shape == y.shape and uvd.shape == uv.shape
    # a pad that pushes the box out of the picture draws nothing
    assert R.masks("x", w, h, halign=0, valign=0, xpad=64, ypad=0) is None


def test_edges_touch_at_pad_zero():
    w, h = 208, 120
    for halign, valign in ((0, 0), (2, 2)):
        T, O, B = R.masks("edge", w, h, halign=halign, valign=valign, xpad=0, ypad=0, scale=1)
        ys, xs = np.nonzero(B)
        assert (xs.min() == 0) == (halign == 0) and (xs.max() == w - 1) == (halign == 2)
        assert (ys.min() == 0) == (valign == 0) and (ys.max() == h - 1) == (valign == 2)


def test_odd_scale_gives_a_chroma_site_per_touched_quad():
    w, h = 200, 112
    y, uv = _pic(w, h)
    T, O, B = R.masks("Hg", w, h, scale=3, xpad=7, ypad=5, halign=0)
    ink = T | O
    # with s = 3 the masks are not aligned to the 2 x 2 quads
    quads = ink.reshape(h // 2, 2, w // 2, 2)
    n = quads.sum(axis=(1, 3))
    assert ((n > 0) & (n < 4)).any()
    yd, uvd = R.draw(y, uv, "Hg", scale=3, xpad=7, ypad=5, halign=0)
    c, c0 = uvd.reshape(h // 2, w // 2, 2), uv.reshape(h // 2, w // 2, 2)
    assert (c[n > 0] == 128).all() and np.array_equal(c[n == 0], c0[n == 0])


def test_text_is_cut_at_255_bytes_and_foreign_bytes_draw_a_question_mark():
    w, h = 64, 48
    y, uv = _pic(w, h)
    long = ("0123456789" * 30)
    a = R.draw(y, uv, long[:255], halign=0, xpad=0, ypad=0, scale=1)
    b = R.draw(y, uv, long, halign=0, xpad=0, ypad=0, scale=1)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    a = R.draw(y, uv, b"a\x80\x07b", halign=0)
    b = R.draw(y, uv, b"a??b", halign=0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert len(LINE) == 53
