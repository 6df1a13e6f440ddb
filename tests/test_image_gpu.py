"""GPU: the image layers (k_image.hip, enc_image.cpp).  The kernels bit for bit against tests/imageref.py, and the invariant
the feature is pinned by: a stream encoded with image layers is byte for byte the stream of the same pictures with the images already blended in
by imageref (and any text drawn afterwards by overlayref), submitted to a plain encoder -- on every submit path, through a recovery, and with the
image replaced and moved while pictures are in flight, also from another thread."""
import ctypes as C
import threading

import numpy as np
import pytest

from oracle import csc
from tests import cscref
from tests import imageref as R
from tests import orientref
from tests import overlayref
from tests import qualityref as Q
from tests import scaleref
from tests.inputref import device_planes
from tests.test_scale_gpu import clip
from tests.util import pad_planes

pytestmark = pytest.mark.gpu

GEOMS = [(64, 48), (200, 112), (208, 120)]  # no margin / right margin 8 / bottom margin 8


def _noise(w, h, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w), dtype=np.uint8)


def _placements(w, h, rng):
    """[(pixels RGBA, x, y)]: the sizes and places the kernel can go wrong at -- one pixel, odd sizes at odd places, negative places, the picture's last
    column / row (and one short of it, at odd offsets), an image that covers the whole picture and more"""
    small, odd, mid, big = R.random_image(rng, 1, 1), R.random_image(rng, 3, 5), R.random_image(rng, 37, 21), R.random_image(rng, w + 40, h + 20)
    return [(small, 5, 7), (odd, 1, 1), (mid, 5, 7), (mid, -3, -4), (mid, w - 10, h - 6), (mid, w - 11, h - 7), (big, -20, -10)]


def _layer(E, pix, x, y, opacity=256, fmt=None):
    fmt = E.FMT_RGBX if fmt is None else fmt
    return E.image_layer(R.to_fmt(pix, fmt), x, y, opacity, fmt)


@pytest.mark.parametrize("matrix,full", [(1, 0), (1, 1), (6, 0), (6, 1)])
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "%dx%d" % g)
def test_stage_image_is_bit_exact(E, geom, matrix, full):
    w, h = geom
    rng = np.random.default_rng(w * 5 + h + matrix + 2 * full)
    y, uv = _noise(w, h, w + h)
    py, puv = pad_planes(y, uv)
    coef = R.coefficients(matrix, full, w, h)
    e = E.Encoder(w, h, fixed_qp=30, colorimetry=(full, 2, 2, matrix))
    changed = 0
    for pix, x, yy in _placements(w, h, rng):
        for opacity in (256, 77, 0):
            for fmt in R.FMTS:
                dy, duv = e.stage_image([_layer(E, pix, x, yy, opacity, fmt)], py, puv)
                ry, ruv = R.blend_coded(y, uv, [R.layer(pix, x, yy, opacity)], coef)
                tag = (pix.shape, x, yy, opacity, fmt)
                assert np.array_equal(dy, ry), (tag, np.argwhere(dy != ry)[:4])
                assert np.array_equal(duv, ruv), (tag, np.argwhere(duv != ruv)[:4])
                if opacity == 0:
                    assert np.array_equal(dy, py) and np.array_equal(duv, puv)
                changed += not np.array_equal(dy, py)
    assert changed >= 7 * 2 * 4 - 8  # (every case with an opacity changes the picture; room for nothing but a lone pixel that happens to match)
    dy, duv = e.stage_image([], py, puv)
    assert np.array_equal(dy, py) and np.array_equal(duv, puv)
    e.close()


@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "%dx%d" % g)
def test_stage_image_blends_layers_in_index_order(E, geom):
    w, h = geom
    rng = np.random.default_rng(w + 3 * h)
    y, uv = _noise(w, h, 17)
    py, puv = pad_planes(y, uv)
    coef = R.coefficients(2, 0, w, h)  # unspecified: BT.601 at these sizes
    # four images that overlap each other around the picture's bottom right corner, odd and even places, two opacities
    spec = [(R.random_image(rng, 37, 21), w - 40, h - 24, 256), (R.random_image(rng, 30, 30), w - 31, h - 29, 200),
            (R.random_image(rng, 21, 37), w - 25, h - 30, 77), (R.random_image(rng, 16, 16), w - 16, h - 16, 256)]
    e = E.Encoder(w, h, fixed_qp=30)
    seen = []
    for order in ([0, 1], [1, 0], [0, 1, 2, 3], [3, 2, 1, 0]):
        ls = [spec[k] for k in order]
        fmts = [R.FMTS[k] for k in order]
        dy, duv = e.stage_image([_layer(E, p, x, yy, op, f) for (p, x, yy, op), f in zip(ls, fmts)], py, puv)
        ry, ruv = R.blend_coded(y, uv, [R.layer(p, x, yy, op) for p, x, yy, op in ls], coef)
        assert np.array_equal(dy, ry), (order, np.argwhere(dy != ry)[:4])
        assert np.array_equal(duv, ruv), (order, np.argwhere(duv != ruv)[:4])
        seen.append(dy)
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[2], seen[3])
    # an entry without pixels is skipped
    dy, duv = e.stage_image([E.image_layer(None), _layer(E, *spec[0])], py, puv)
    ry, ruv = R.blend_coded(y, uv, [R.layer(*spec[0])], coef)
    assert np.array_equal(dy, ry) and np.array_equal(duv, ruv)
    e.close()


@pytest.mark.parametrize("geom,place", [((208, 120), (208 - 10, 120 - 6)), ((208, 120), (208 - 11, 120 - 7)), ((200, 112), (200 - 10, 112 - 6)), ((200, 112), (200 - 11, 112 - 7)),
                                        ((200, 112), (-20, -10))])
def test_margin_is_written_from_the_blended_samples_not_read(E, geom, place):
    """Noise in the margin.  Where the launch's grid -- the visible intersection from an even origin, so whole quads -- reaches the last visible column (row), the
    margin beside (below) those rows (columns) repeats the blended last column (row), chroma the last pair (row); the noise stays everywhere else."""
    w, h = geom
    W, H = (w + 15) // 16 * 16, (h + 15) // 16 * 16
    y, uv = _noise(w, h, 5)
    py, puv = _noise(W, H, 6)
    py[:h, :w], puv[:h // 2, :w] = y, uv
    rng = np.random.default_rng(7)
    pix = R.random_image(rng, 37, 21) if place[0] >= 0 else R.random_image(rng, w + 40, h + 20)
    x, yy = place
    e = E.Encoder(w, h, fixed_qp=30)
    dy, duv = e.stage_image([_layer(E, pix, x, yy, 200)], py, puv)
    e.close()
    ry, ruv = R.blend(y, uv, [R.layer(pix, x, yy, 200)], R.coefficients(2, 0, w, h))
    assert np.array_equal(dy[:h, :w], ry) and np.array_equal(duv[:h // 2, :w], ruv)
    gx0, gy0 = max(x, 0) & ~1, max(yy, 0) & ~1
    assert min(x + pix.shape[1], w) == w and min(yy + pix.shape[0], h) == h  # (the image reaches both last lines)
    ey, euv = py.copy(), puv.copy()
    ey[:h, :w], euv[:h // 2, :w] = ry, ruv
    ey[gy0:h, w:] = ry[gy0:h, w - 1:w]                  # right of the grid's rows
    ey[h:, gx0:w] = ry[h - 1:h, gx0:w]                  # below the grid's columns
    ey[h:, w:] = ry[h - 1, w - 1]                       # the corner
    cpair = ruv.reshape(h // 2, w // 2, 2)
    euv.reshape(H // 2, W // 2, 2)[gy0 // 2:h // 2, w // 2:] = cpair[gy0 // 2:, w // 2 - 1:w // 2]
    euv[h // 2:, gx0:w] = ruv[h // 2 - 1:h // 2, gx0:w]
    euv.reshape(H // 2, W // 2, 2)[h // 2:, w // 2:] = cpair[h // 2 - 1, w // 2 - 1]
    assert np.array_equal(dy, ey), np.argwhere(dy != ey)[:4]
    assert np.array_equal(duv, euv), np.argwhere(duv != euv)[:4]


def test_a_handle_validates_its_layers(E):
    w, h = 64, 48
    e = E.Encoder(w, h, fixed_qp=30)
    img = np.zeros((4, 6, 4), np.uint8)
    assert e.last_image(0) == (0, 0, 0, 0, 0, 0) and e.image_bytes() == 0
    with pytest.raises(E.EncoderError, match=r"\(%d\)" % E.ERR_STATE):
        e.set_image_place(0, 1, 1)  # the layer is off
    with pytest.raises(E.EncoderError, match=r"\(%d\)" % E.ERR_STATE):
        e.time_stage(E.STAGE_IMAGE, 1)  # no image on layer 0
    e.set_image(3, img, -16384, 16384, 0, E.FMT_XBGR)
    e.set_image_place(3, 16384, -16384, 256)
    bad = [dict(layer=4), dict(layer=-1), dict(fmt=E.FMT_BGR), dict(fmt=E.FMT_NV12), dict(x=16385), dict(x=-16385), dict(y=16385), dict(y=-16385), dict(opacity=257), dict(opacity=-1)]
    for b in bad:
        kw = dict(dict(layer=0, x=0, y=0, opacity=256, fmt=E.FMT_RGBX), **b)
        with pytest.raises(E.EncoderError, match=r"\(%d\)" % E.ERR_ARG):
            e.set_image(kw.pop("layer"), img, **kw)
    for x, yy, op in ((16385, 0, 256), (0, -16385, 256), (0, 0, 257), (0, 0, -1)):
        with pytest.raises(E.EncoderError, match=r"\(%d\)" % E.ERR_ARG):
            e.set_image_place(3, x, yy, op)
    L = e.L
    for fld, v in (("w", 0), ("w", 4097), ("h", 0), ("h", 4097), ("stride", 23)):
        im = E.image_layer(img)
        setattr(im, fld, v)
        assert L.mi355enc_set_image(e.h, 0, C.byref(im)) == E.ERR_ARG, (fld, v)
    assert L.mi355enc_last_image(e.h, 4, C.byref(E.ImageInfo())) == E.ERR_ARG
    # the handle stayed as it was: layer 0 off, layer 3 as set; switching off counts as a call
    with pytest.raises(E.EncoderError, match=r"\(%d\)" % E.ERR_STATE):
        e.set_image_place(0, 1, 1)
    e.set_image(0, img)
    e.set_image(0, None)
    y, uv = _noise(w, h, 1)
    e.submit(y, uv)
    e.collect()
    assert e.last_image(0) == (0, 0, 0, 0, 0, 0) and e.last_image(3) == (6, 4, 16384, -16384, 256, 1)
    assert e.image_bytes() == 0  # (layer 3 lies outside the picture: nothing was uploaded)
    e.set_image(0, img)
    e.submit(y, uv)
    e.collect()
    assert e.last_image(0) == (6, 4, 0, 0, 256, 3) and e.image_bytes() >= 4 * 6 * 4
    # rows at a stride of their own
    wide = np.random.default_rng(2).integers(0, 256, (4, 10, 4), dtype=np.uint8)
    dy, duv = e.stage_image([E.image_layer(wide[:, 2:8], 3, 3)], *pad_planes(y, uv))
    ry, ruv = R.blend_coded(y, uv, [R.layer(wide[:, 2:8], 3, 3)], R.coefficients(2, 0, w, h))
    assert np.array_equal(dy, ry) and np.array_equal(duv, ruv)
    e.close()


def test_a_matrix_rgb_cannot_be_converted_with_refuses_the_picture(E):
    w, h = 64, 48
    y, uv = _noise(w, h, 1)
    e = E.Encoder(w, h, fixed_qp=30, colorimetry=(0, 2, 2, 0))  # GBR: no matrix to convert with
    e.submit(y, uv)
    e.collect()
    e.set_image(1, np.full((4, 4, 4), 255, np.uint8), opacity=0)
    e.submit(y, uv)  # (opacity 0: not an active layer)
    e.collect()
    e.set_image_place(1, 0, 0, 1)
    with pytest.raises(E.EncoderError, match=r"\(%d\)" % E.ERR_ARG):
        e.submit(y, uv)
    assert e.pending == 0
    e.set_image(1, None)
    e.submit(y, uv)
    e.collect()
    e.close()


# ---- streams: 5 pictures, gop 3, fixed QP, three in flight; two layers, the first one moving with every picture
N, QP, GOP = 5, 28, 3
STYLE = dict(xpad=0, ypad=0, scale=1, shaded_background=1)
TEXTS = ["  b: %5d/%5.0f rtt: %3d" % (2048 - 100 * i, 1900.0 + 7 * i, 40 + i) for i in range(N)]


def _layers(w, h, i, seed=21):
    """what picture i carries: layer 0 a 37 x 21 image that moves from outside the top left corner across odd and even places, layer 2 a 16 x 16 one in the bottom
    right corner (it touches both margins) at opacity 77"""
    rng = np.random.default_rng(seed)
    a, b = R.random_image(rng, 37, 21), R.random_image(rng, 16, 16)
    return {0: (a, -5 + 7 * i, -3 + 5 * i, 256), 2: (b, w - 16, h - 16, 77)}


def _ref_layers(spec):
    return [R.layer(*spec[k]) for k in sorted(spec)]


def run(e, feed, n, before=None, depth=2):
    """-> [(au, key, pts, qp, (last_image of the four layers))]"""
    out = []

    def take():
        out.append(e.collect() + (tuple(e.last_image(l) for l in range(4)),))
    for i in range(n):
        if before:
            before(i)
        feed(i)
        if e.pending > depth:
            take()
    while e.pending:
        take()
    return out


def plain_stream(E, w, h, pictures, before=None, **kw):
    """the stream of visible-size NV12 pictures from an encoder that knows nothing of images"""
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=2, **kw)
    out = run(e, lambda i: e.submit(pictures[i][0], pictures[i][1], pts=i), len(pictures), before=(lambda i: before(e, i)) if before else None)
    assert e.image_bytes() == 0
    e.close()
    assert all(o[4] == ((0,) * 6,) * 4 for o in out)
    return out


def same(got, ref):
    assert len(got) == len(ref)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g[0] == r[0] and g[1:4] == r[1:4], (i, len(g[0]), len(r[0]))


def image_encoder(E, w, h, **kw):
    return E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=2, **kw)


def place_layers(E, e, w, h, i):
    """the layers of picture i on encoder e: the images once, then only the place of layer 0"""
    spec = _layers(w, h, i)
    if i == 0:
        for k, (p, x, yy, op) in spec.items():
            f = R.FMTS[k]
            e.set_image(k, R.to_fmt(p, f), x, yy, op, f)
    else:
        e.set_image_place(0, *spec[0][1:])


def blended(w, h, sources, texts=None):
    coef = R.coefficients(2, 0, w, h)
    out = []
    for i, (y, uv) in enumerate(sources):
        p = R.blend(y[:h, :w], uv[:h // 2, :w], _ref_layers(_layers(w, h, i)), coef)
        out.append(overlayref.draw(p[0], p[1], texts[i], **STYLE) if texts else p)
    return out


def check_reports(got, w, h):
    for i, g in enumerate(got):
        spec = _layers(w, h, i)
        assert g[4][0] == (37, 21) + spec[0][1:] + (1,) and g[4][2] == (16, 16) + spec[2][1:] + (1,) and g[4][1] == g[4][3] == (0,) * 6, (i, g[4])


@pytest.mark.parametrize("geom", [(208, 120), (200, 112)], ids=lambda g: "%dx%d" % g)
def test_stream_from_host_nv12(E, oracle, geom):
    w, h = geom
    pics = clip(w, h, N)
    ref = plain_stream(E, w, h, blended(w, h, pics))
    e = image_encoder(E, w, h)
    got = run(e, lambda i: e.submit(*pics[i], pts=i), N, before=lambda i: place_layers(E, e, w, h, i))
    dec = oracle.Decoder()
    for g in got:
        dy, duv = dec.decode(g[0])
    assert np.array_equal(dy, e.fetch(E.FETCH_RECON_Y)) and np.array_equal(duv, e.fetch(E.FETCH_RECON_UV))
    assert e.image_bytes() >= 4 * (37 * 21 + 16 * 16)
    e.close()
    same(got, ref)
    check_reports(got, w, h)
    # ... and from the blocking entry point, one picture at a time
    e, p = E.Encoder(w, h, gop=GOP, fixed_qp=QP), E.Encoder(w, h, gop=GOP, fixed_qp=QP)
    src = blended(w, h, pics)
    for i in range(3):
        place_layers(E, e, w, h, i)
        assert e.encode(*pics[i], pts=i) == p.encode(*src[i], pts=i), i
    e.close(); p.close()


def test_stream_from_yuy2(E):
    w, h = 200, 112
    rng = np.random.default_rng(11)
    planes = [cscref.random_planes(E.FMT_YUY2, w, h, rng) for _ in range(N)]
    sources = [csc.to_nv12(csc.FMT_YUY2, p, w, h) for p in planes]
    ref = plain_stream(E, w, h, blended(w, h, sources))
    e = image_encoder(E, w, h)
    got = run(e, lambda i: e.submit_fmt(E.FMT_YUY2, planes[i], pts=i), N, before=lambda i: place_layers(E, e, w, h, i))
    e.close()
    same(got, ref)
    check_reports(got, w, h)


def test_stream_from_scaled_input(E):
    """400 x 224 -> 200 x 112: the image is blended after the scale, at the coded size -- it is never scaled"""
    iw, ih, w, h = 400, 224, 200, 112
    pics = clip(iw, ih, N)
    sources = [scaleref.to_nv12(scaleref.FMT_NV12, [y, uv], iw, ih, w, h) for y, uv in pics]
    ref = plain_stream(E, w, h, blended(w, h, sources))
    e = image_encoder(E, w, h, input_size=(iw, ih))
    got = run(e, lambda i: e.submit(*pics[i], pts=i), N, before=lambda i: place_layers(E, e, w, h, i))
    e.close()
    same(got, ref)


def test_stream_through_a_transposing_orientation_keeps_the_image_upright(E):
    w, h = 200, 112
    pics = clip(h, w, N)  # submitted 112 wide, 200 high; turned right on the device
    sources = [orientref.orient(y, uv, 1) for y, uv in pics]
    ref = plain_stream(E, w, h, blended(w, h, sources))
    e = image_encoder(E, w, h, orientation="90r")
    got = run(e, lambda i: e.submit(*pics[i], pts=i), N, before=lambda i: place_layers(E, e, w, h, i))
    e.close()
    same(got, ref)


def test_stream_with_a_text_overlay_on_top(E):
    w, h = 208, 120
    pics = clip(w, h, N)
    ref = plain_stream(E, w, h, blended(w, h, pics, TEXTS))
    e = image_encoder(E, w, h)
    e.set_overlay_style(**STYLE)

    def before(i):
        place_layers(E, e, w, h, i)
        e.set_overlay_text(TEXTS[i])
    got = run(e, lambda i: e.submit(*pics[i], pts=i), N, before=before)
    e.close()
    same(got, ref)


def test_stream_with_the_adaptive_transform_and_adaptive_quantisation(E):
    w, h = 208, 120
    pics = clip(w, h, N)
    kw = dict(transform8x8=2, aq=True)
    ref = plain_stream(E, w, h, blended(w, h, pics), **kw)
    e = image_encoder(E, w, h, **kw)
    got = run(e, lambda i: e.submit(*pics[i], pts=i), N, before=lambda i: place_layers(E, e, w, h, i))
    e.close()
    same(got, ref)


def test_submit_device_blends_into_its_own_copy_and_leaves_the_callers_planes(E):
    """aligned planes at a stride of 16 n: without a layer the kernels read them in place; with one they are copied, and never written"""
    w, h = 208, 112
    pics = clip(w, h, N)
    ref = plain_stream(E, w, h, blended(w, h, pics))
    dev = [device_planes(E, [y, uv], [h, h // 2], [w, w], w, 0) for y, uv in pics]
    e = image_encoder(E, w, h)
    got = run(e, lambda i: e.submit_device(dev[i][2][0], w, dev[i][2][1], w, pts=i), N, before=lambda i: place_layers(E, e, w, h, i))
    e.close()
    for (hip, buf, _), (y, uv) in zip(dev, pics):
        back = np.empty(w * h * 3 // 2, np.uint8)
        assert hip.hipMemcpy(back.ctypes.data_as(C.c_void_p), buf, C.c_size_t(back.size), 2) == 0  # hipMemcpyDeviceToHost
        assert np.array_equal(back[:w * h].reshape(h, w), y) and np.array_equal(back[w * h:].reshape(h // 2, w), uv)
        hip.hipFree(buf)
    same(got, ref)


def test_quality_metrics_measure_against_the_blended_source(E, oracle):
    w, h = 200, 112
    pics = clip(w, h, N)
    src = blended(w, h, pics)
    e = image_encoder(E, w, h)
    e.set_quality_metrics(True)
    dec = oracle.Decoder()
    for i in range(N):  # one at a time: the metrics of picture i against the decoder's output of its access unit
        place_layers(E, e, w, h, i)
        e.submit(*pics[i], pts=i)
        dy, duv = dec.decode(e.collect()[0])
        assert e.last_quality().ints() == Q.quality(src[i][0], src[i][1], dy, duv, w, h), i
    e.close()


def test_off_is_off(E):
    w, h = 208, 120
    pics = clip(w, h, N)
    ref = plain_stream(E, w, h, pics)
    img = R.random_image(np.random.default_rng(1), 37, 21)
    e = image_encoder(E, w, h)  # never set
    got = run(e, lambda i: e.submit(*pics[i], pts=i), N)
    assert e.image_bytes() == 0
    e.close()
    same(got, ref)
    e = image_encoder(E, w, h)  # set, then cleared before the first submit
    e.set_image(0, img, 5, 7)
    e.set_image(0, None)
    got = run(e, lambda i: e.submit(*pics[i], pts=i), N)
    assert e.image_bytes() == 0 and all(g[4] == ((0,) * 6,) * 4 for g in got)
    e.close()
    same(got, ref)
    e = image_encoder(E, w, h)  # opacity 0
    e.set_image(0, img, 5, 7, opacity=0)
    got = run(e, lambda i: e.submit(*pics[i], pts=i), N)
    assert e.image_bytes() == 0 and all(g[4][0] == (37, 21, 5, 7, 0, 1) for g in got)
    e.close()
    same(got, ref)
    e = image_encoder(E, w, h)  # an image that is transparent everywhere
    e.set_image(0, img * np.array([1, 1, 1, 0], np.uint8), 5, 7)
    got = run(e, lambda i: e.submit(*pics[i], pts=i), N)
    e.close()
    same(got, ref)


def test_recovery_does_not_blend_twice(E):
    """Opacity 77 (blending it twice would show), three pictures in flight when the tripped word is seen: the pictures come back through recover(), which enqueues
    their surfaces again -- with the images already in them.  The plain encoder goes through the same trip."""
    w, h, n = 208, 120, 7
    pics = clip(w, h, n)
    img = R.random_image(np.random.default_rng(3), 60, 40)
    coef = R.coefficients(2, 0, w, h)
    src = [R.blend(y, uv, [R.layer(img, 9 + i, 11, 77)], coef) for i, (y, uv) in enumerate(pics)]
    trip = lambda e, i: e.debug_trip_wait(12) if i == 3 else None
    ref = plain_stream(E, w, h, src, before=trip)
    e = image_encoder(E, w, h)

    def before(i):
        trip(e, i)
        e.set_image(0, img, 9 + i, 11, 77) if i == 0 else e.set_image_place(0, 9 + i, 11, 77)
    got = run(e, lambda i: e.submit(*pics[i], pts=i), n, before=before)
    st = e.stats()
    e.close()
    assert st.recoveries == 1 and got[3][1]  # (the first picture in flight came back as an IDR picture)
    same(got, ref)
    assert [g[4][0] for g in got] == [(60, 40, 9 + i, 11, 77, 1) for i in range(n)]


def test_image_replaced_and_moved_with_pictures_in_flight(E):
    """three pictures in flight; before every submit the image is replaced (three images of three sizes in turn, the third switching the layer off) or moved: every
    picture is the blend with what last_image reports for it, and the reports are what was set before its submit"""
    w, h, n = 208, 120, 9
    pics = clip(w, h, n)
    rng = np.random.default_rng(4)
    imgs = [R.random_image(rng, 37, 21), R.random_image(rng, 64, 48), None, R.random_image(rng, 8, 100)]
    coef = R.coefficients(2, 0, w, h)
    e = image_encoder(E, w, h)
    by_serial, want = {}, []
    serial = 0

    def before(i):
        nonlocal serial
        x, yy, op = 3 * i - 4, 2 * i + 1, 256 - 20 * i
        if i % 2 == 0:
            img = imgs[(i // 2) % 4]
            e.set_image(0, img, x, yy, op)
            serial += 1
            by_serial[serial] = img
        elif by_serial[serial] is not None:
            e.set_image_place(0, x, yy, op)
        else:
            x, yy, op = want[-1][2:5]
        img = by_serial[serial]
        want.append((img.shape[1], img.shape[0], x, yy, op, serial) if img is not None else (0,) * 6)
    got = run(e, lambda i: e.submit(*pics[i], pts=i), n, before=before)
    peak = e.image_bytes()
    e.close()
    assert [g[4][0] for g in got] == want
    src = [R.blend(y, uv, [R.layer(by_serial[r[5]], r[2], r[3], r[4])] if r[5] else [], coef) for (y, uv), r in zip(pics, want)]
    same(got, plain_stream(E, w, h, src))
    assert 0 < peak <= 4 * 4 * (37 * 21 + 64 * 48 + 8 * 100)  # (retired buffers are used again: never more than a few of each size)


def test_image_replaced_from_another_thread_is_latched_whole(E):
    """two opaque images of one colour each, flipped by another thread while this one submits: every picture carries the one its report's serial names, whole"""
    w, h, n = 208, 120, 12
    pics = clip(w, h, 4)
    a, b = np.empty((40, 56, 4), np.uint8), np.empty((40, 56, 4), np.uint8)
    a[:], b[:] = (255, 0, 0, 255), (0, 0, 255, 255)
    e = image_encoder(E, w, h)
    e.set_image(0, a, 11, 9)  # serial 1; the thread's k-th call makes serial k + 2 and sets (b, a)[k & 1]
    stop = threading.Event()

    def flip():
        k = 0
        while not stop.is_set():
            e.set_image(0, (b, a)[k & 1], 11, 9)
            k += 1
    th = threading.Thread(target=flip)
    th.start()
    try:
        got = run(e, lambda i: e.submit(*pics[i % 4], pts=i), n)
    finally:
        stop.set()
        th.join()
    e.close()
    coef = R.coefficients(2, 0, w, h)
    src = []
    for i, g in enumerate(got):
        rep = g[4][0]
        assert rep[:5] == (56, 40, 11, 9, 256) and rep[5] >= 1, rep
        img = a if rep[5] % 2 == 1 else b  # serial 1 a, 2 b, 3 a, ...
        src.append(R.blend(*pics[i % 4], [R.layer(img, 11, 9)], coef))
    same(got, plain_stream(E, w, h, src))


def test_time_stage_runs_the_blend_launch(E):
    w, h = 208, 120
    e = E.Encoder(w, h, fixed_qp=30)
    e.set_image(0, R.random_image(np.random.default_rng(1), 64, 64), 10, 10)
    ms = e.time_stage(E.STAGE_IMAGE, 3)
    assert ms > 0 and e.image_bytes() >= 4 * 64 * 64
    print("image blend launch, 64 x 64 layer at %d x %d: %.4f ms" % (w, h, ms))
    e.close()
