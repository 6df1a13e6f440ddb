"""GPU: orientation of the input picture (k_orient.hip, enc_orient.cpp).  The kernel bit for bit against tests/orientref.py
plus the margin rule of tests/util.pad_planes, and the invariant the feature is pinned by: the stream of an oriented encoder fed P is byte for byte
the stream of a plain encoder fed orientref(P) -- on every submit path, scaled, under the overlay, with metrics, through a recovery."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import csc
from tests import cscref
from tests import orientref as R
from tests import overlayref
from tests import qualityref as Q
from tests import scaleref
from tests import spsref
from tests.inputref import device_planes

pytestmark = pytest.mark.gpu

GEOMS = R.GEOMS
METHODS = range(8)
N, QP, GOP = 5, 28, 3
STREAM_GEOMS = [(72, 40), (208, 120)]
STREAM_METHODS = [1, 2, 7]
JPEG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg", "q50_420_72x40.jpg")


def gid(g):
    return "%dx%d" % g


def source(w, h, method, seed):
    """a noise picture of the pre-orientation size of a coded w x h picture"""
    pw, ph = R.size(method, w, h)
    return R.noise(pw, ph, seed)


def strided(a, extra, fill):
    """`a` as a view into a wider array of `fill` noise: row stride = width + extra"""
    wide = np.random.default_rng(fill).integers(0, 256, (a.shape[0], a.shape[1] + extra), dtype=np.uint8)
    wide[:, :a.shape[1]] = a
    return wide[:, :a.shape[1]]


# ---- 1: the kernel against the reference, tight and at strides that are no multiple of 4
@pytest.mark.parametrize("geom", GEOMS, ids=gid)
def test_stage_orient_is_bit_exact(E, geom):
    w, h = geom
    e = E.Encoder(w, h, fixed_qp=30)
    for m in range(1, 8):
        y, uv = source(w, h, m, 100 * m + w)
        ry, ruv = R.orient_coded(y, uv, m)
        assert ry.shape == (e.mbh * 16, e.mbw * 16)
        for extra in (0, 7, 33):
            sy, suv = (y, uv) if not extra else (strided(y, extra, 1), strided(uv, extra + 2, 2))
            assert not extra or (sy.strides[0] % 4 and suv.strides[0] % 4 and sy.strides[0] != suv.strides[0])
            dy, duv = e.stage_orient(m, sy, suv)
            assert np.array_equal(dy, ry), (R.NAMES[m], extra, np.argwhere(dy != ry)[:4])
            assert np.array_equal(duv, ruv), (R.NAMES[m], extra, np.argwhere(duv != ruv)[:4])
    with pytest.raises(E.EncoderError, match=r"\(%d\)" % E.ERR_ARG):
        e.stage_orient(0, *source(w, h, 0, 1))  # identity is no launch
    with pytest.raises(E.EncoderError, match=r"\(%d\)" % E.ERR_ARG):
        e.stage_orient(8, *source(w, h, 0, 1))
    e.close()


# ---- 2, 3: device planes at odd addresses and strides; guard bands around the output and the input; the margin is written, not read
def _device_run(E, e, m, y, uv, stride, offset, out_offset, poison_seed):
    """-> (out container before, after, input container before, after, offsets)"""
    ph, pw = y.shape
    H, W = e.mbh * 16, e.mbw * 16
    hip, buf, ptrs = device_planes(E, [y, uv], [ph, ph // 2], [pw, pw], stride, offset)
    in_size = offset + (ph + ph // 2) * stride
    before_in = np.empty(in_size, np.uint8)
    assert hip.hipMemcpy(before_in.ctypes.data_as(C.c_void_p), buf, C.c_size_t(in_size), 2) == 0
    guard = 4096
    out = np.random.default_rng(poison_seed).integers(0, 256, 2 * guard + out_offset + W * H * 3 // 2 + guard, dtype=np.uint8)
    dout = C.c_void_p()
    assert hip.hipMalloc(C.byref(dout), C.c_size_t(out.size)) == 0
    assert hip.hipMemcpy(dout, out.ctypes.data_as(C.c_void_p), C.c_size_t(out.size), 1) == 0
    oy = guard + out_offset
    ouv = oy + W * H + guard  # a guard band between the two surfaces as well
    e.stage_orient_device(m, ptrs[0], stride, ptrs[1], stride, dout.value + oy, dout.value + ouv)
    after = np.empty_like(out)
    assert hip.hipMemcpy(after.ctypes.data_as(C.c_void_p), dout, C.c_size_t(out.size), 2) == 0
    after_in = np.empty_like(before_in)
    assert hip.hipMemcpy(after_in.ctypes.data_as(C.c_void_p), buf, C.c_size_t(in_size), 2) == 0
    hip.hipFree(buf)
    hip.hipFree(dout)
    return out, after, before_in, after_in, oy, ouv


@pytest.mark.parametrize("geom", GEOMS, ids=gid)
def test_stage_orient_device_on_unaligned_planes_with_guard_bands(E, geom):
    w, h = geom
    e = E.Encoder(w, h, fixed_qp=30)
    H, W = e.mbh * 16, e.mbw * 16
    for m in range(1, 8):
        y, uv = source(w, h, m, 7 * m + h)
        ry, ruv = R.orient_coded(y, uv, m)
        for stride_extra, offset, out_offset in ((0, 0, 0), (13, 3, 0), (1, 1, 16), (16, 16, 5)):  # aligned / odd both / odd / aligned input into an unaligned surface
            out, after, bin_, ain, oy, ouv = _device_run(E, e, m, y, uv, y.shape[1] + stride_extra, offset, out_offset, 40 + m)
            case = (R.NAMES[m], stride_extra, offset, out_offset)
            assert np.array_equal(after[oy:oy + W * H].reshape(H, W), ry), case
            assert np.array_equal(after[ouv:ouv + W * H // 2].reshape(H // 2, W), ruv), case
            keep = np.ones(out.size, bool)
            keep[oy:oy + W * H] = False
            keep[ouv:ouv + W * H // 2] = False
            assert np.array_equal(after[keep], out[keep]), case  # nothing around the surfaces is written
            assert np.array_equal(ain, bin_), case  # the caller's planes are only read
    e.close()


@pytest.mark.parametrize("method", [1, 2, 5, 7], ids=[R.NAMES[m] for m in (1, 2, 5, 7)])
def test_margin_is_written_from_the_held_samples_not_read(E, method):
    """18 x 34 has a margin on both axes.  Two runs over two different poisons in the output margin give the same surfaces, and those are the reference's:
    the margin comes from the visible samples, whatever lay there before."""
    w, h = 18, 34
    e = E.Encoder(w, h, fixed_qp=30)
    y, uv = source(w, h, method, 9)
    ry, ruv = R.orient_coded(y, uv, method)
    H, W = e.mbh * 16, e.mbw * 16
    got = []
    for poison in (1, 2):
        out, after, _, _, oy, ouv = _device_run(E, e, method, y, uv, y.shape[1], 0, 0, poison)
        py = out[oy:oy + W * H].reshape(H, W)
        assert not np.array_equal(py[h:], ry[h:]) and not np.array_equal(py[:, w:], ry[:, w:])  # (the poison is not the answer)
        got.append((after[oy:oy + W * H].reshape(H, W), after[ouv:ouv + W * H // 2].reshape(H // 2, W)))
    for dy, duv in got:
        assert np.array_equal(dy, ry) and np.array_equal(duv, ruv)
    e.close()


# ---- streams
def run(e, feed, n, depth=2, before=None):
    """-> [(au, key, pts, qp)], and the reconstruction fetched after the last picture"""
    out = []
    for i in range(n):
        if before:
            before(i)
        feed(i)
        if e.pending > depth:
            out.append(e.collect())
    while e.pending:
        out.append(e.collect())
    return out, (e.fetch(0), e.fetch(1))  # MI355ENC_FETCH_RECON_Y, MI355ENC_FETCH_RECON_UV


def plain_stream(E, w, h, oriented, before=None, **kw):
    """the stream of already-oriented pictures from an encoder that knows nothing of orientation"""
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=2, **kw)
    res = run(e, lambda i: e.submit(oriented[i][0], oriented[i][1], pts=i), len(oriented), before=(lambda i: before(e, i)) if before else None)
    st = e.stats()
    e.close()
    return res, st


def oriented_encoder(E, w, h, method, **kw):
    return E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=2, orientation=method, **kw)


def same(got, ref):
    (ga, grec), (ra, rrec) = got, ref
    assert len(ga) == len(ra)
    for i, (g, r) in enumerate(zip(ga, ra)):
        assert g == r, (i, len(g[0]), len(r[0]), g[1:], r[1:])
    assert np.array_equal(grec[0], rrec[0]) and np.array_equal(grec[1], rrec[1])


def clips(w, h, method, seed=0):
    """N pre-orientation pictures (the first noise, the rest a drifting copy with fresh noise mixed in: P pictures with work to do) and their oriented forms"""
    pw, ph = R.size(method, w, h)
    base = R.noise(pw, ph, 50 + seed)
    pics = []
    for i in range(N):
        fresh = R.noise(pw, ph, 60 + seed + i)
        y = np.where(fresh[0] < 40, fresh[0], np.roll(base[0], 2 * i, axis=1))
        uv = np.where(fresh[1] % 8 == 0, fresh[1], np.roll(base[1], 2 * i, axis=1))
        pics.append((np.ascontiguousarray(y), np.ascontiguousarray(uv)))
    return pics, [R.orient(y, uv, method) for y, uv in pics]


@pytest.mark.parametrize("method", STREAM_METHODS, ids=[R.NAMES[m] for m in STREAM_METHODS])
@pytest.mark.parametrize("geom", STREAM_GEOMS, ids=gid)
def test_stream_from_host_nv12(E, oracle, geom, method):
    w, h = geom
    pics, oriented = clips(w, h, method)
    ref, _ = plain_stream(E, w, h, oriented)
    e = oriented_encoder(E, w, h, method)
    assert e.get_orientation() == method and e.input_size == R.size(method, w, h)
    got = run(e, lambda i: e.submit(*pics[i], pts=i), N)
    st = e.stats()
    assert e.orient_bytes() > 0
    e.close()
    same(got, ref)
    assert st.pinned_inputs == 0
    dec = oracle.Decoder()  # ... and it is a stream: the decoder's last picture is the reconstruction
    for au in got[0]:
        dy, duv = dec.decode(au[0])
    assert np.array_equal(dy, got[1][0]) and np.array_equal(duv, got[1][1])
    # from mi355enc_host_alloc memory: transferred in place
    pw, ph = R.size(method, w, h)
    per = pw * ph * 3 // 2
    buf = E.PinnedBuffer(N * per)
    views = []
    for i, (y, uv) in enumerate(pics):
        a = buf.array[i * per:(i + 1) * per]
        a[:pw * ph] = y.ravel()
        a[pw * ph:] = uv.ravel()
        views.append((a[:pw * ph].reshape(ph, pw), a[pw * ph:].reshape(ph // 2, pw)))
    e = oriented_encoder(E, w, h, method)
    got = run(e, lambda i: e.submit(*views[i], pts=i), N)
    st = e.stats()
    e.close()
    del views, a
    buf.free()
    same(got, ref)
    assert st.pinned_inputs == N
    # the blocking entry point
    e, p = E.Encoder(w, h, gop=GOP, fixed_qp=QP, orientation=R.NAMES[method]), E.Encoder(w, h, gop=GOP, fixed_qp=QP)
    for i in range(3):
        assert e.encode(*pics[i], pts=i) == p.encode(*oriented[i], pts=i), i
    e.close(); p.close()


@pytest.mark.parametrize("fmt", ["yuy2", "bgrx"])
@pytest.mark.parametrize("method", STREAM_METHODS, ids=[R.NAMES[m] for m in STREAM_METHODS])
@pytest.mark.parametrize("geom", STREAM_GEOMS, ids=gid)
def test_stream_from_converted_input(E, geom, method, fmt):
    w, h = geom
    pw, ph = R.size(method, w, h)
    f = E.FMT_YUY2 if fmt == "yuy2" else E.FMT_BGRX
    rng = np.random.default_rng(11 + method)
    planes = [cscref.random_planes(f, pw, ph, rng) for _ in range(N)]
    nv12 = [(csc.to_nv12(csc.FMT_YUY2, p, pw, ph) if f == E.FMT_YUY2 else cscref.to_nv12(f, p, pw, ph)) for p in planes]
    oriented = [R.orient(y[:ph, :pw], uv[:ph // 2, :pw], method) for y, uv in nv12]
    ref, _ = plain_stream(E, w, h, oriented)
    e = oriented_encoder(E, w, h, method)
    got = run(e, lambda i: e.submit_fmt(f, planes[i], pts=i), N)
    e.close()
    same(got, ref)


@pytest.mark.parametrize("method", STREAM_METHODS, ids=[R.NAMES[m] for m in STREAM_METHODS])
@pytest.mark.parametrize("geom", STREAM_GEOMS, ids=gid)
def test_stream_from_device_planes_is_never_in_place(E, geom, method):
    """aligned planes at a stride of 16 n: the plain path would read them in place; oriented, they are read where they lie and never written"""
    w, h = geom
    pics, oriented = clips(w, h, method, seed=3)
    ref, _ = plain_stream(E, w, h, oriented)
    pw, ph = R.size(method, w, h)
    stride = (pw + 15) // 16 * 16
    dev = [device_planes(E, [y, uv], [ph, ph // 2], [pw, pw], stride, 0) for y, uv in pics]
    e = oriented_encoder(E, w, h, method)
    got = run(e, lambda i: e.submit_device(dev[i][2][0], stride, dev[i][2][1], stride, pts=i), N)
    e.close()
    for (hip, buf, _), (y, uv) in zip(dev, pics):
        back = np.empty(stride * ph * 3 // 2, np.uint8)
        assert hip.hipMemcpy(back.ctypes.data_as(C.c_void_p), buf, C.c_size_t(back.size), 2) == 0  # hipMemcpyDeviceToHost
        assert np.array_equal(back[:stride * ph].reshape(ph, stride)[:, :pw], y) and np.array_equal(back[stride * ph:].reshape(ph // 2, stride)[:, :pw], uv)
        hip.hipFree(buf)
    same(got, ref)


@pytest.mark.parametrize("method", STREAM_METHODS, ids=[R.NAMES[m] for m in STREAM_METHODS])
def test_stream_from_jpeg(E, method):
    """the golden 72 x 40 picture is the pre-orientation input: the encoder is 40 x 72 for the transposing methods"""
    data = open(JPEG, "rb").read()
    w, h = R.size(method, 72, 40)
    d = E.Encoder(72, 40, fixed_qp=30)
    jy, juv = d.stage_jpeg(data)  # (the decode itself is pinned by tests/test_jpeg_gpu.py)
    d.close()
    oriented = [R.orient(jy[:40, :72], juv[:20, :72], method)] * N
    ref, _ = plain_stream(E, w, h, oriented)
    e = oriented_encoder(E, w, h, method)
    got = run(e, lambda i: e.submit_jpeg(data, pts=i), N)
    e.close()
    same(got, ref)
    if method in R.TRANSPOSING:  # a picture of the oriented size is refused, and leaves nothing behind
        e = oriented_encoder(E, 72, 40, method)
        with pytest.raises(E.EncoderError, match=r"\(%d\)" % E.ERR_ARG):
            e.submit_jpeg(data)
        assert e.pending == 0
        e.close()


# ---- 5: scaled input
def _sps_sar(au):
    return spsref.sps_of(au)[0]["sar"]


@pytest.mark.parametrize("insize,sar", [((144, 80), None), ((144, 120), (3, 2))], ids=["144x80", "144x120"])
def test_scaled_input_is_scaled_to_the_pre_orientation_size_then_oriented(E, insize, sar):
    """-> 72 x 40 -> 90l -> coded 40 x 72.  144 x 80 keeps the aspect ratio (no SAR, as the scaler alone); 144 x 120 makes the scaler's 2:3, written as 3:2"""
    iw, ih = insize
    w, h, m = 40, 72, 3
    rng = np.random.default_rng(21)
    pics = [(rng.integers(0, 256, (ih, iw), dtype=np.uint8), rng.integers(0, 256, (ih // 2, iw), dtype=np.uint8)) for _ in range(N)]
    scaled = [scaleref.to_nv12(scaleref.FMT_NV12, [y, uv], iw, ih, 72, 40) for y, uv in pics]
    oriented = [R.orient(y[:40, :72], uv[:20, :72], m) for y, uv in scaled]
    ref, _ = plain_stream(E, w, h, oriented)
    e = oriented_encoder(E, w, h, m, input_size=(iw, ih))
    got = run(e, lambda i: e.submit(*pics[i], pts=i), N)
    e.close()
    plain_sar = _sps_sar(ref[0][0][0])
    assert plain_sar is None
    assert _sps_sar(got[0][0][0]) == sar
    if sar is None:
        same(got, ref)
    else:  # the SPS differs by the VUI's aspect ratio alone: the slices and the reconstruction are the plain encoder's
        assert np.array_equal(got[1][0], ref[1][0]) and np.array_equal(got[1][1], ref[1][1])
        for g, r in zip(got[0], ref[0]):
            gs = [n for n in spsref.nal_units(g[0]) if n[0] in (1, 5)]
            rs = [n for n in spsref.nal_units(r[0]) if n[0] in (1, 5)]
            assert gs == rs and g[1:] == r[1:]
        s = E.Encoder(72, 40, gop=GOP, fixed_qp=QP, input_size=(iw, ih))  # the scaler alone writes the same ratio the other way round
        au, _ = s.encode(*pics[0])
        s.close()
        assert _sps_sar(au) == sar[::-1]


def test_scaled_jpeg_and_scaled_device_planes_are_oriented_too(E):
    """the two other scaled routes into the pre-orientation picture: 72 x 40 JPEG -> 36 x 20 -> 90r -> coded 20 x 36, and device planes 144 x 80 -> 72 x 40 -> ur-ll"""
    data = open(JPEG, "rb").read()
    d = E.Encoder(72, 40, fixed_qp=30)
    jy, juv = d.stage_jpeg(data)
    d.close()
    sy, suv = scaleref.to_nv12(scaleref.FMT_NV12, [np.ascontiguousarray(jy[:40, :72]), np.ascontiguousarray(juv[:20, :72])], 72, 40, 36, 20)
    oriented = [R.orient(sy[:20, :36], suv[:10, :36], 1)] * N
    ref, _ = plain_stream(E, 20, 36, oriented)
    e = oriented_encoder(E, 20, 36, 1, input_size=(72, 40))
    got = run(e, lambda i: e.submit_jpeg(data, pts=i), N)
    e.close()
    same(got, ref)
    iw, ih, w, h, m = 144, 80, 40, 72, 7
    rng = np.random.default_rng(31)
    pics = [(rng.integers(0, 256, (ih, iw), dtype=np.uint8), rng.integers(0, 256, (ih // 2, iw), dtype=np.uint8)) for _ in range(N)]
    scaled = [scaleref.to_nv12(scaleref.FMT_NV12, [y, uv], iw, ih, 72, 40) for y, uv in pics]
    ref, _ = plain_stream(E, w, h, [R.orient(y[:40, :72], uv[:20, :72], m) for y, uv in scaled])
    dev = [device_planes(E, [y, uv], [ih, ih // 2], [iw, iw], iw + 5, 3) for y, uv in pics]
    e = oriented_encoder(E, w, h, m, input_size=(iw, ih))
    got = run(e, lambda i: e.submit_device(dev[i][2][0], iw + 5, dev[i][2][1], iw + 5, pts=i), N)
    e.close()
    for hip, buf, _ in dev:
        hip.hipFree(buf)
    same(got, ref)


# ---- 6: the overlay is drawn after the orientation (the text stays upright)
@pytest.mark.parametrize("method", [1, 2], ids=["90r", "180"])
def test_overlay_is_drawn_on_the_oriented_picture(E, method):
    w, h = 208, 120
    style = dict(xpad=0, ypad=0, scale=1, shaded_background=1)
    text = "b: 2048 rtt: 40"
    pics, oriented = clips(w, h, method, seed=5)
    drawn = [overlayref.draw(y, uv, text, **style) for y, uv in oriented]
    ref, _ = plain_stream(E, w, h, drawn)
    e = oriented_encoder(E, w, h, method)
    e.set_overlay_style(**style)
    e.set_overlay_text(text)
    got = run(e, lambda i: e.submit(*pics[i], pts=i), N)
    e.close()
    same(got, ref)
    # ... and the surfaces themselves: draw_coded applied after orientref
    cy, cuv = overlayref.draw_coded(oriented[0][0], oriented[0][1], text, **style)
    e = E.Encoder(w, h, fixed_qp=30)
    sy, suv = e.stage_orient(method, *pics[0])
    dy, duv = e.stage_overlay(text, sy, suv, **style)
    e.close()
    assert np.array_equal(dy, cy) and np.array_equal(duv, cuv)


# ---- 7: metrics against the oriented source
def test_quality_metrics_measure_against_the_oriented_source(E, oracle):
    w, h, m = 72, 40, 1
    pics, oriented = clips(w, h, m, seed=7)
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, orientation=m)
    e.set_quality_metrics(True)
    dec = oracle.Decoder()
    for i in range(N):
        e.submit(*pics[i], pts=i)
        dy, duv = dec.decode(e.collect()[0])
        assert e.last_quality().ints() == Q.quality(oriented[i][0], oriented[i][1], dy, duv, w, h), i
    e.close()


# ---- 8: off is off
def test_off_is_off(E):
    w, h = 208, 120
    pics, _ = clips(w, h, 0)
    ref, _ = plain_stream(E, w, h, pics)
    for how in ("keyword", "setter", "set and cleared"):
        e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=2, orientation=0 if how == "keyword" else None)
        if how == "setter":
            e.set_orientation("identity")
        if how == "set and cleared":
            e.set_orientation("90r")
            e.set_orientation(0)
        got = run(e, lambda i: e.submit(*pics[i], pts=i), N)
        assert e.orient_bytes() == 0 and e.get_orientation() == 0 and e.input_size == (w, h), how
        e.close()
        same(got, ref)
    # the in-place device path stays in place: nothing is copied, so nothing is allocated for it either
    dev = [device_planes(E, [y, uv], [h, h // 2], [w, w], w, 0) for y, uv in pics]
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=2, orientation=0)
    got = run(e, lambda i: e.submit_device(dev[i][2][0], w, dev[i][2][1], w, pts=i), N)
    assert e.orient_bytes() == 0
    e.close()
    for hip, buf, _ in dev:
        hip.hipFree(buf)
    same(got, ref)


# ---- 9: a recovery re-encodes the oriented surfaces; it does not orient again
def test_recovery_does_not_orient_twice(E):
    w, h, m, n = 208, 120, 1, 7
    pics, oriented = clips(w, h, m, seed=9)
    pics, oriented = (pics + pics[:2])[:n], (oriented + oriented[:2])[:n]
    trip = lambda e, i: e.debug_trip_wait(12) if i == 3 else None
    ref, rst = plain_stream(E, w, h, oriented, before=trip)
    e = oriented_encoder(E, w, h, m)
    got = run(e, lambda i: e.submit(*pics[i], pts=i), n, before=lambda i: trip(e, i))
    st = e.stats()
    e.close()
    assert st.recoveries == 1 and rst.recoveries == 1 and got[0][3][1]  # (the first picture in flight came back as an IDR picture)
    same(got, ref)


# ---- 10: setter states
def test_setter_states(E):
    w, h = 40, 72
    pics, oriented = clips(w, h, 3, seed=11)
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP)
    for bad in (8, -1):
        with pytest.raises(E.EncoderError, match=r"\(%d\)" % E.ERR_ARG):
            e.set_orientation(bad)
    assert e.get_orientation() == 0
    e.set_orientation(3)
    e.submit(*pics[0])
    with pytest.raises(E.EncoderError, match=r"\(%d\)" % E.ERR_STATE):
        e.set_orientation(0)
    e.collect()
    with pytest.raises(E.EncoderError, match=r"\(%d\)" % E.ERR_STATE):
        e.set_orientation(1)
    assert e.get_orientation() == 3
    e.close()


def test_either_order_of_the_two_setters_gives_the_same_stream(E):
    iw, ih, w, h, m = 144, 120, 40, 72, 3
    rng = np.random.default_rng(23)
    pics = [(rng.integers(0, 256, (ih, iw), dtype=np.uint8), rng.integers(0, 256, (ih // 2, iw), dtype=np.uint8)) for _ in range(N)]
    out = []
    for order in ("orientation first", "size first"):
        e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=2)
        if order == "orientation first":
            e.set_orientation(m)
            e.set_input_size(iw, ih)
        else:
            e.set_input_size(iw, ih)  # (fits the unoriented target 40 x 72 as well: 144 <= 8 * 40)
            e.set_orientation(m)
        out.append(run(e, lambda i: e.submit(*pics[i], pts=i), N))
        e.close()
    same(out[0], out[1])
    assert _sps_sar(out[0][0][0][0]) == (3, 2)


def test_a_refused_combination_leaves_the_handle_usable(E):
    """coded 40 x 72: an input of 60 x 72 fits the plain target (60 -> 40 wide) but not the target of a transposing method, 72 x 40 (60 < 72)"""
    w, h = 40, 72
    pics, oriented = clips(w, h, 0, seed=13)
    ref, _ = plain_stream(E, w, h, pics)
    # the size is set first, the orientation completes the refused pair
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=2)
    e.set_input_size(40, 72)
    e.set_input_size(60, 72)  # scales 60 -> 40 wide: fine without a method
    with pytest.raises(E.EncoderError, match=r"\(%d\)" % E.ERR_ARG):
        e.set_orientation(1)  # the target becomes 72 x 40: 60 < 72
    assert e.get_orientation() == 0
    e.set_input_size(40, 72)  # ... and the handle is as it was: back to the unscaled path, it codes the plain stream
    got = run(e, lambda i: e.submit(*pics[i], pts=i), N)
    e.close()
    same(got, ref)
    # the orientation is set first, the size completes the refused pair
    pics3, oriented3 = clips(w, h, 3, seed=13)
    ref3, _ = plain_stream(E, w, h, oriented3)
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=2, orientation=3)
    with pytest.raises(E.EncoderError, match=r"\(%d\)" % E.ERR_ARG):
        e.set_input_size(60, 72)
    assert e.get_orientation() == 3 and e.input_size == (72, 40)
    got = run(e, lambda i: e.submit(*pics3[i], pts=i), N)
    e.close()
    same(got, ref3)
