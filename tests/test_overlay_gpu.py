"""GPU: the text overlay (k_overlay.hip, enc_overlay.cpp).  The kernel bit for bit against tests/overlayref.py, and the
invariant the feature is pinned by: a stream encoded with an overlay is byte for byte the stream of the same pictures with the text already
drawn into them by overlayref, submitted to a plain encoder -- on every submit path, through a recovery, and with the text changing from
another thread."""
import ctypes as C
import threading

import numpy as np
import pytest

from oracle import csc
from tests import cscref
from tests import overlayref as R
from tests import qualityref as Q
from tests import scaleref
from tests.inputref import device_planes
from tests.test_scale_gpu import clip
from tests.util import pad_planes

pytestmark = pytest.mark.gpu

LINE = "  b:  2048/ 1900 rtt:  40/ 38/ 45 bs:  12/ 10/ 14/ 11"  # the reference's statistics line
GEOMS = [(64, 48), (208, 120), (200, 112), (198, 118), (1920, 1080)]  # no margin / bottom / right / both, odd macroblock remainder / the flagship size


def _cases(w, h):
    out = [(LINE, dict(scale=s)) for s in (1, 2, 3, 0)]
    for ha in range(3):
        for va in range(3):
            # pad 0: the drawing touches the picture's edges, and so the margin
            out.append(("edge %d%d" % (ha, va), dict(halign=ha, valign=va, xpad=0, ypad=0, scale=1 + (ha + va) % 3, shaded_background=(ha + va) & 1)))
    out.append(("Hg", dict(halign=2, valign=2, xpad=0, ypad=0, scale=3, shaded_background=1)))
    out.append(("Hg", dict(halign=2, valign=2, xpad=0, ypad=0, scale=2, shaded_background=0)))
    out.append(("two lines\nof text, the second longer", dict(halign=1, valign=1, shaded_background=1)))
    out.append(("right\naligned lines\n\nx", dict(halign=2, valign=2, xpad=6, ypad=10, scale=1)))
    out.append(("W" * (w // 8 + 9), dict(halign=2, xpad=0, ypad=0, scale=1, shaded_background=1)))  # wider than the picture
    out.append(("0123456789" * 25 + "abcde", dict(halign=0, valign=2, xpad=3, ypad=1, scale=1)))  # 255 bytes
    out.append(("0123456789" * 30, dict(halign=0, valign=2, xpad=3, ypad=1, scale=1, shaded_background=1)))  # 300 bytes: cut at 255
    out.append((b"caf\xe9 \x80\xff\x07 ok", dict(halign=0, valign=0, xpad=1, ypad=1)))  # bytes outside the font
    out.append(("\n".join("line %d" % i for i in range(h // 16 + 3)), dict(halign=0, valign=0, xpad=0, ypad=0, scale=1, shaded_background=1)))  # higher than the picture
    return out


@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "%dx%d" % g)
def test_stage_overlay_is_bit_exact(E, geom):
    w, h = geom
    rng = np.random.default_rng(w * 3 + h)
    y, uv = rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w), dtype=np.uint8)
    py, puv = pad_planes(y, uv)
    e = E.Encoder(w, h, fixed_qp=30)
    for text, st in _cases(w, h):
        dy, duv = e.stage_overlay(text, py, puv, **st)
        ry, ruv = R.draw_coded(y, uv, text, **st)
        assert np.array_equal(dy, ry), (text, st, np.argwhere(dy != ry)[:4])
        assert np.array_equal(duv, ruv), (text, st, np.argwhere(duv != ruv)[:4])
        assert not np.array_equal(dy, py)
    dy, duv = e.stage_overlay("", py, puv)
    assert np.array_equal(dy, py) and np.array_equal(duv, puv)
    e.close()


def test_margin_is_written_from_the_drawn_samples_not_read(E):
    """208 x 120: the width is a multiple of 16, so no submit path pads the bottom margin before the launch.  With noise there, a shaded box that touches
    the last visible row leaves the drawn last row (chroma: the last chroma row) in the margin rows of its columns, and the noise everywhere else."""
    w, h = 208, 120
    rng = np.random.default_rng(5)
    y, uv = rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w), dtype=np.uint8)
    py, puv = rng.integers(0, 256, (128, w), dtype=np.uint8), rng.integers(0, 256, (64, w), dtype=np.uint8)
    py[:h], puv[:h // 2] = y, uv
    st = dict(halign=1, valign=2, xpad=0, ypad=0, scale=1, shaded_background=1)
    e = E.Encoder(w, h, fixed_qp=30)
    dy, duv = e.stage_overlay("margin", py, puv, **st)
    e.close()
    ry, ruv = R.draw(y, uv, "margin", **st)
    _, _, B = R.masks("margin", w, h, **st)
    cols = B[h - 1]
    assert cols.any() and not cols.all() and not (cols[0::2] ^ cols[1::2]).any()
    assert np.array_equal(dy[:h], ry) and np.array_equal(duv[:h // 2], ruv)
    assert (dy[h:, cols] == ry[h - 1, cols]).all() and np.array_equal(dy[h:, ~cols], py[h:, ~cols])
    assert (duv[h // 2:, cols] == ruv[h // 2 - 1, cols]).all() and np.array_equal(duv[h // 2:, ~cols], puv[h // 2:, ~cols])


def test_a_handle_validates_the_style(E):
    e = E.Encoder(64, 48, fixed_qp=30)
    e.set_overlay_style(halign=0, valign=2, xpad=0, ypad=100, scale=8, shaded_background=1)
    for bad in (dict(halign=3), dict(halign=-1), dict(valign=3), dict(xpad=-1), dict(ypad=-2), dict(scale=9), dict(scale=-1), dict(shaded_background=2)):
        with pytest.raises(E.EncoderError, match=r"\(%d\)" % E.ERR_ARG):
            e.set_overlay_style(**bad)
    with pytest.raises(E.EncoderError, match=r"\(%d\)" % E.ERR_STATE):  # nothing collected yet
        e.last_overlay()
    e.close()


# ---- streams: 5 pictures, gop 4, fixed QP, three in flight, the text changing with every picture
N, QP = 5, 28
TEXTS = ["  b: %5d/%5.0f rtt: %3d/%3d/%3d bs: %3d/%3d/%3d/%3d" % (2048 - 100 * i, 1900.0 + 7 * i, 40 + i, 38, 45 + 2 * i, 12, 10 + i, 14, 11) for i in range(N)]
STYLE = dict(xpad=0, ypad=0, scale=1, shaded_background=1)  # right, top, touching both edges


def run(e, feed, n, texts=None, depth=2, before=None):
    """-> [(au, key, pts, qp, last_overlay)]"""
    out = []

    def take():
        out.append(e.collect() + (e.last_overlay(),))
    for i in range(n):
        if before:
            before(i)
        if texts is not None:
            e.set_overlay_text(texts[i])
        feed(i)
        if e.pending > depth:
            take()
    while e.pending:
        take()
    return out


def plain_stream(E, w, h, sources, texts, style, before=None, **kw):
    """the stream of `sources` (coded- or visible-size NV12) with texts[i] drawn in by overlayref, from an encoder that knows nothing of overlays"""
    drawn = [R.draw(y[:h, :w], uv[:h // 2, :w], t, **style) for (y, uv), t in zip(sources, texts)]
    e = E.Encoder(w, h, gop=4, fixed_qp=QP, pipeline_depth=2, **kw)
    out = run(e, lambda i: e.submit(drawn[i][0], drawn[i][1], pts=i), len(drawn), before=(lambda i: before(e, i)) if before else None)
    e.close()
    assert all(o[4] == b"" for o in out)
    return out, drawn


def overlay_encoder(E, w, h, style, **kw):
    e = E.Encoder(w, h, gop=4, fixed_qp=QP, pipeline_depth=2, **kw)
    e.set_overlay_style(**style)
    return e


def same(got, ref, texts):
    assert len(got) == len(ref)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g[0] == r[0] and g[1:4] == r[1:4], (i, len(g[0]), len(r[0]))
        assert g[4] == R.as_bytes(texts[i]), i


@pytest.mark.parametrize("geom", [(208, 120), (200, 112)], ids=lambda g: "%dx%d" % g)
def test_stream_from_host_nv12(E, oracle, geom):
    w, h = geom
    pics = clip(w, h, N)
    ref, _ = plain_stream(E, w, h, pics, TEXTS, STYLE)
    e = overlay_encoder(E, w, h, STYLE)
    got = run(e, lambda i: e.submit(*pics[i], pts=i), N, TEXTS)
    dec = oracle.Decoder()
    for g in got:
        dy, duv = dec.decode(g[0])
    assert np.array_equal(dy, e.fetch(E.FETCH_RECON_Y)) and np.array_equal(duv, e.fetch(E.FETCH_RECON_UV))
    e.close()
    same(got, ref, TEXTS)
    # ... and from the blocking entry point, one picture at a time
    e = E.Encoder(w, h, gop=4, fixed_qp=QP)
    e.set_overlay_style(**STYLE)
    p = E.Encoder(w, h, gop=4, fixed_qp=QP)
    for i in range(3):
        e.set_overlay_text(TEXTS[i])
        assert e.encode(*pics[i], pts=i) == p.encode(*R.draw(pics[i][0], pics[i][1], TEXTS[i], **STYLE), pts=i), i
    e.close(); p.close()


@pytest.mark.parametrize("fmt", ["yuy2", "bgrx"])
def test_stream_from_converted_input(E, fmt):
    w, h = 200, 112
    f = E.FMT_YUY2 if fmt == "yuy2" else E.FMT_BGRX
    rng = np.random.default_rng(11)
    planes = [cscref.random_planes(f, w, h, rng) for _ in range(N)]
    sources = [(csc.to_nv12(csc.FMT_YUY2, p, w, h) if f == E.FMT_YUY2 else cscref.to_nv12(f, p, w, h)) for p in planes]
    ref, _ = plain_stream(E, w, h, sources, TEXTS, STYLE)
    e = overlay_encoder(E, w, h, STYLE)
    got = run(e, lambda i: e.submit_fmt(f, planes[i], pts=i), N, TEXTS)
    e.close()
    same(got, ref, TEXTS)


def test_stream_from_scaled_input(E):
    """640 x 480 -> 320 x 240: the text is drawn after the scale, at the coded size -- it is never scaled down"""
    iw, ih, w, h = 640, 480, 320, 240
    pics = clip(iw, ih, N)
    sources = [scaleref.to_nv12(scaleref.FMT_NV12, [y, uv], iw, ih, w, h) for y, uv in pics]
    ref, _ = plain_stream(E, w, h, sources, TEXTS, STYLE)
    e = overlay_encoder(E, w, h, STYLE, input_size=(iw, ih))
    got = run(e, lambda i: e.submit(*pics[i], pts=i), N, TEXTS)
    e.close()
    same(got, ref, TEXTS)


def test_submit_device_draws_into_its_own_copy_and_leaves_the_callers_planes(E):
    """aligned planes at a stride of 16 n: without a text the kernels read them in place; with one they are copied, and never written"""
    w, h = 208, 112
    pics = clip(w, h, N)
    ref, _ = plain_stream(E, w, h, pics, TEXTS, STYLE)
    dev = [device_planes(E, [y, uv], [h, h // 2], [w, w], w, 0) for y, uv in pics]
    e = overlay_encoder(E, w, h, STYLE)
    got = run(e, lambda i: e.submit_device(dev[i][2][0], w, dev[i][2][1], w, pts=i), N, TEXTS)
    e.close()
    for (hip, buf, _), (y, uv) in zip(dev, pics):
        back = np.empty(w * h * 3 // 2, np.uint8)
        assert hip.hipMemcpy(back.ctypes.data_as(C.c_void_p), buf, C.c_size_t(back.size), 2) == 0  # hipMemcpyDeviceToHost
        assert np.array_equal(back[:w * h].reshape(h, w), y) and np.array_equal(back[w * h:].reshape(h // 2, w), uv)
        hip.hipFree(buf)
    same(got, ref, TEXTS)


def test_stream_with_the_high_profile_toolset_and_adaptive_quantisation(E):
    w, h = 208, 120
    pics = clip(w, h, N)
    kw = dict(transform8x8=2, i8x8=True, aq=True)
    ref, _ = plain_stream(E, w, h, pics, TEXTS, STYLE, **kw)
    e = overlay_encoder(E, w, h, STYLE, **kw)
    got = run(e, lambda i: e.submit(*pics[i], pts=i), N, TEXTS)
    e.close()
    same(got, ref, TEXTS)


def test_quality_metrics_measure_against_the_overlaid_source(E, oracle):
    w, h = 200, 112
    pics = clip(w, h, N)
    e = overlay_encoder(E, w, h, STYLE)
    e.set_quality_metrics(True)
    dec = oracle.Decoder()
    for i in range(N):  # one at a time: the metrics of picture i against the decoder's output of its access unit
        e.set_overlay_text(TEXTS[i])
        e.submit(*pics[i], pts=i)
        au = e.collect()[0]
        dy, duv = dec.decode(au)
        sy, suv = R.draw(pics[i][0], pics[i][1], TEXTS[i], **STYLE)
        assert e.last_quality().ints() == Q.quality(sy, suv, dy, duv, w, h), i
    e.close()


def test_off_is_off(E):
    w, h = 208, 120
    pics = clip(w, h, N)
    ref, _ = plain_stream(E, w, h, pics, [""] * N, {})
    e = overlay_encoder(E, w, h, STYLE)
    e.set_overlay_text("")
    got = run(e, lambda i: e.submit(*pics[i], pts=i), N)
    e.close()
    same(got, ref, [""] * N)
    e = overlay_encoder(E, w, h, STYLE)
    e.set_overlay_text(LINE)
    e.set_overlay_text(None)  # cleared again before the first submit
    got = run(e, lambda i: e.submit(*pics[i], pts=i), N)
    e.close()
    same(got, ref, [""] * N)


def test_recovery_does_not_draw_twice(E):
    """Shaded background (drawing it twice would halve the box again), three pictures in flight when the tripped word is seen: the pictures come
    back through recover(), which enqueues their surfaces again -- with the text already in them.  The plain encoder goes through the same trip."""
    w, h, n = 208, 120, 7
    pics = clip(w, h, n)
    texts = ["trip %d %s" % (i, LINE[:30]) for i in range(n)]
    trip = lambda e, i: e.debug_trip_wait(12) if i == 3 else None
    ref, _ = plain_stream(E, w, h, pics, texts, STYLE, before=trip)
    e = overlay_encoder(E, w, h, STYLE)
    got = run(e, lambda i: e.submit(*pics[i], pts=i), n, texts, before=lambda i: trip(e, i))
    st = e.stats()
    e.close()
    assert st.recoveries == 1 and got[3][1]  # (the first picture in flight came back as an IDR picture)
    same(got, ref, texts)


def test_text_set_from_another_thread_is_latched_whole(E):
    w, h, n = 208, 120, 12
    pics = clip(w, h, 4)
    a, b = b"A" * 200, b"b: 1\nrtt 2"
    e = overlay_encoder(E, w, h, STYLE)
    e.set_overlay_text(a)
    stop = threading.Event()

    def flip():
        k = 0
        while not stop.is_set():
            e.set_overlay_text((a, b)[k & 1])
            k += 1
    th = threading.Thread(target=flip)
    th.start()
    try:
        got = run(e, lambda i: e.submit(*pics[i % 4], pts=i), n)
    finally:
        stop.set()
        th.join()
    e.close()
    seen = [g[4] for g in got]
    assert all(s in (a, b) for s in seen), seen
    ref, _ = plain_stream(E, w, h, [pics[i % 4] for i in range(n)], seen, STYLE)
    same(got, ref, seen)
